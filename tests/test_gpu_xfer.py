"""modimizer_amd/csrc/mg_xfer.hip piece by piece: mgXferD2H (copy and the saturating 16-bit add), mgXferH2D and mgXferH2DSparse, driven
through the probe library (oracle/xfer_probe.hip -> oracle/libxferprobe.so, which is LINKED against libmodgpu.so: the code that runs is
the library's own), and the public mgCopyD2HBig / mgCopyH2DBig.  Every result the library hands back crosses this file, and its callers
move arrays of less than one 4 MiB piece in the ordinary tests, or check sums behind a prefix in the full-size ones.  Here the pieces are
64 KiB (MODGPU_XFER_PIECE_KB, the smallest the knob takes) and the lengths sit around one piece, T pieces and the first reuse of a
lane's blocks, for 1 to 16 threads; the pointers are off their alignment; the saturating add meets 65535 and 65536 on both sides of a
piece edge; and the sparse upload is given ranges with holes of pages that were never written, and ranges that are not private
anonymous memory.

Device memory is written and read back with mgMemcpyH2D / mgMemcpyD2H, the runtime's own copy, never with the code under test.  The
contents are seeded random bytes, so a piece that is exchanged, repeated or dropped shows.  Every destination lies between fences that
are asserted untouched; the fence BEHIND a buffer is a piece long, so a last piece moved at full length would land in it.  mgXferDiag
(util.xfer_diag) says how many threads and pieces a transfer took and which way a sparse upload went: a case that names four threads is
known to have run on four lanes.  Bytes and integers only: every comparison is exact."""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest

import modimizer_amd as mg
import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(ROOT, "oracle", "libxferprobe.so")
PROBE_SOURCES = ["xfer_probe.hip", "../modimizer_amd/csrc/mg_xfer.h", "../modimizer_amd/csrc/mg_common.h"]
PROBE_MARKER = "XFER_PROBE_HASH"

MG_XFER_COPY, MG_XFER_SATADD16 = 0, 1      # mg_xfer.h
P = 64 << 10                   # MODGPU_XFER_PIECE_KB=64: the smallest piece the knob accepts (mg_xfer.hip, mgXferPrepareLocked)
DEFAULT_PIECE = 4 << 20
SPARSE_FLOOR = 4 << 20         # mgXferH2DSparse looks at the page map from here up
FRONT, BACK = 64, P            # the fences of a buffer: bytes in front of it and behind it
HOST_FENCE, DEV_FENCE, BLANK = 0xEE, 0xDD, 0x5A
PAGE = os.sysconf("SC_PAGESIZE")
THREADS = [1, 2, 3, 4, 16]


# ---- the probe ----------------------------------------------------------------------------------

def probe_source_hash():
    """the hash oracle/Makefile bakes into the probe, over its three sources"""
    return util.probe_source_hash(PROBE_SOURCES)


def probe_binary_hash(path=None):
    """the hash a built probe carries, read out of the file (no dlopen); None if there is no such file or marker"""
    return util.probe_binary_hash(path or PROBE_PATH, PROBE_MARKER)


def build_probe():
    """make the probe if the one in the tree is not the build of the tree's sources"""
    return util.build_probe("libxferprobe.so", PROBE_MARKER, PROBE_SOURCES)


_probe = None


def probe():
    global _probe
    if _probe is None:
        mg.lib()                                         # first: the probe's libmodgpu.so IS the one the package has loaded
        X = C.CDLL(build_probe())
        X.xferProbeHash.restype = C.c_char_p
        if X.xferProbeHash().decode() != probe_source_hash():
            raise RuntimeError("libxferprobe.so (%s) is not the build of this tree's xfer_probe.hip, mg_xfer.h and mg_common.h (%s)"
                               % (X.xferProbeHash().decode(), probe_source_hash()))
        vp, u64 = C.c_void_p, C.c_uint64
        for name, res, args in (("xferProbeD2H", C.c_int, [vp, vp, u64, C.c_int]), ("xferProbeH2D", C.c_int, [vp, vp, u64]),
                                ("xferProbeH2DSparse", C.c_int, [vp, vp, u64]), ("xferProbeMapAnon", vp, [u64]),
                                ("xferProbeMapShared", vp, [u64]), ("xferProbeMapFile", vp, [u64, u64]),
                                ("xferProbeMapHalfFile", vp, [u64, u64]), ("xferProbePageOut", C.c_int, [vp, u64]),
                                ("xferProbeUnmap", C.c_int, [vp, u64]), ("xferProbePresentPages", C.c_long, [vp, u64, vp])):
            f = getattr(X, name); f.restype = res; f.argtypes = args
        _probe = X
    return _probe


def test_probe_is_the_build_of_this_tree():
    X = probe()
    assert X.xferProbeHash().decode() == probe_source_hash() == probe_binary_hash()


# ---- knobs, buffers, the census -------------------------------------------------------------------

@contextlib.contextmanager
def team(threads=None, piece_kb=None, streams=None, release=True):
    """the transfers' knobs for the block.  release: mgReleaseBuffers () on the way in and out, so that the lanes (their streams above
    all: a lane keeps the one it was made with) are made anew under these knobs and the next test's under its own"""
    L = mg.lib()
    if release:
        L.mgReleaseBuffers()
    try:
        with mg.knobs(XFER_THREADS=threads, XFER_PIECE_KB=piece_kb, XFER_STREAMS=streams):
            yield
    finally:
        if release:
            L.mgReleaseBuffers()


class HostArea:
    """n bytes at `off` bytes behind a 64-byte line, FRONT + off bytes of fence in front at least and BACK behind"""

    def __init__(self, n, off, content=None, fence=HOST_FENCE):
        self.n, self.fence = n, fence
        self.whole = np.full(FRONT + 64 + off + n + BACK, fence, np.uint8)
        self.start = (-self.whole.ctypes.data) % 64 + FRONT + off
        assert (self.whole.ctypes.data + self.start) % 64 == off % 64
        self.view = self.whole[self.start:self.start + n]
        self.view[:] = BLANK if content is None else content
        self.addr = self.whole.ctypes.data + self.start

    def fences_intact(self):
        return bool(np.all(self.whole[:self.start] == self.fence) and np.all(self.whole[self.start + self.n:] == self.fence))


class DevArea:
    """one device allocation that serves every case of a test: set () lays fence, n bytes and fence at its start with the runtime's own
    copy, read () brings the whole of that back the same way"""

    def __init__(self, nmax, offmax=16):
        self.buf = mg.DeviceBuffer(FRONT + offmax + nmax + BACK)
        self.cap = self.buf.nbytes

    def set(self, n, off, content=None):
        self.n, self.start = n, FRONT + off
        image = np.full(self.start + n + BACK, DEV_FENCE, np.uint8)
        assert len(image) <= self.cap
        image[self.start:self.start + n] = BLANK if content is None else content
        mg.check(mg.lib().mgMemcpyH2D(self.buf.ptr, image.ctypes.data, image.nbytes, None))
        mg.check(mg.lib().mgStreamSynchronize(None))
        self.addr = self.buf.ptr.value + self.start
        return self

    def read(self):
        """(the n bytes, fences intact)"""
        image = self.buf.to_numpy(np.uint8, self.start + self.n + BACK)
        return (image[self.start:self.start + self.n],
                bool(np.all(image[:self.start] == DEV_FENCE) and np.all(image[self.start + self.n:] == DEV_FENCE)))

    def free(self):
        self.buf.free()


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return "%d wrong, first at byte %d (piece %d of 64 KiB, byte %d of it): %#x, not %#x" % (
        len(bad), bad[0], bad[0] // P, bad[0] % P, int(got[bad[0]]), int(want[bad[0]]))


def census_of_one(before, after, nbytes, threads, piece, what):
    """one transfer of nbytes: ceil (nbytes / piece) pieces on min (threads, pieces) lanes; none at all for no bytes"""
    if nbytes == 0:
        assert after == before, what
        return
    pieces = -(-nbytes // piece)
    want = dict(before, transfers=before["transfers"] + 1, pieces=before["pieces"] + pieces, threads=min(threads, pieces), piece_bytes=piece)
    assert after == want, what + (after, want)


def upload(X, dev, data, n, hoff, doff, threads, piece, what, call=None):
    """data[:n] from a host array at hoff into the device at doff through the team, read back plainly"""
    src = HostArea(n, hoff, data[:n])
    kept = src.whole.copy()
    dev.set(n, doff)
    before = util.xfer_diag()
    rc = (call or X.xferProbeH2D)(dev.addr, src.addr, n)
    after = util.xfer_diag()
    assert rc == 0, what + (mg.lib().mgLastError(),)
    got, fences = dev.read()
    if not np.array_equal(got, data[:n]):
        raise AssertionError(what + (first_difference(got, data[:n]),))
    assert fences, what + ("device bytes outside the destination were written",)
    assert np.array_equal(src.whole, kept), what + ("the host source was changed",)
    census_of_one(before, after, n, threads, piece, what)


def download(X, dev, data, n, hoff, doff, threads, piece, what, call=None):
    """data[:n], put on the device at doff plainly, into a host array at hoff through the team"""
    dev.set(n, doff, data[:n])
    dst = HostArea(n, hoff)
    before = util.xfer_diag()
    rc = call(dst.addr, dev.addr, n) if call else X.xferProbeD2H(dst.addr, dev.addr, n, MG_XFER_COPY)
    after = util.xfer_diag()
    assert rc == 0, what + (mg.lib().mgLastError(),)
    if not np.array_equal(dst.view, data[:n]):
        raise AssertionError(what + (first_difference(dst.view, data[:n]),))
    assert dst.fences_intact(), what + ("host bytes outside the destination were written",)
    got, fences = dev.read()
    assert fences and np.array_equal(got, data[:n]), what + ("the device source was changed",)
    census_of_one(before, after, n, threads, piece, what)


def copy_lengths(t):
    """around one piece, around t pieces (every lane one piece), 2t pieces and one byte (every lane both of its blocks), the first reuse of
    a block (the first event wait of the upload), and a ragged set of lanes"""
    return list(dict.fromkeys([0, 1, P - 1, P, P + 1, 2 * P + 1, t * P - 1, t * P, t * P + 1, 2 * t * P + 1, 3 * t * P + P // 2 + 1, (3 * t + 1) * P + 3]))


def run_copies(t, streams):
    X = probe()
    lengths = copy_lengths(t)
    data = np.random.default_rng(7000 + t).integers(0, 256, max(lengths), dtype=np.uint8)
    dev = DevArea(max(lengths))
    with team(t, 64, streams):
        for n in lengths:
            for hoff in (0, 1):                          # the callers pass ms->info + 1
                for doff in (0, 1, 16):                  # and dNc + 1 (16 bytes), t.value + first
                    what = ("T %d" % t, "streams %s" % streams, "%d bytes" % n, "host + %d" % hoff, "device + %d" % doff)
                    upload(X, dev, data, n, hoff, doff, t, P, what + ("H2D",))
                    download(X, dev, data, n, hoff, doff, t, P, what + ("D2H",))
    dev.free()


# ---- copies in both directions --------------------------------------------------------------------

@pytest.mark.parametrize("t", THREADS)
def test_copies_both_ways(t):
    """H2D then a plain read-back is the source; a plain upload then D2H is the source; nothing outside the destination is written, the
    source stays what it was, no bytes move nothing, and the census shows min (T, pieces) threads and ceil (bytes / P) pieces"""
    run_copies(t, None)


def test_copies_on_the_default_stream():
    """the same with MODGPU_XFER_STREAMS=0: the lanes' copies and events on the device's default stream"""
    run_copies(4, 0)


def test_copies_at_the_default_piece():
    """the production setting: 4 MiB pieces, the default team, 9 MiB + 5 bytes (two whole pieces and a short one)"""
    X = probe()
    n = (9 << 20) + 5
    data = np.random.default_rng(9).integers(0, 256, n, dtype=np.uint8)
    dev = DevArea(n)
    with team():
        t = mg.lib().mgXferThreadCount()
        assert 1 <= t <= 16
        upload(X, dev, data, n, 1, 16, t, DEFAULT_PIECE, ("default piece", "H2D"))
        download(X, dev, data, n, 1, 16, t, DEFAULT_PIECE, ("default piece", "D2H"))
    dev.free()


def test_public_big_copies():
    """mgCopyH2DBig / mgCopyD2HBig (include/modgpu.h): one round trip of ten pieces and a bit on three lanes"""
    X = probe()
    L = mg.lib()
    n = 10 * P + 4321
    data = np.random.default_rng(10).integers(0, 256, n, dtype=np.uint8)
    dev = DevArea(n)
    with team(3, 64):
        upload(X, dev, data, n, 1, 1, 3, P, ("mgCopyH2DBig",), call=L.mgCopyH2DBig)
        download(X, dev, data, n, 1, 1, 3, P, ("mgCopyD2HBig",), call=L.mgCopyD2HBig)
    dev.free()


def test_piece_size_and_team_change_in_one_process():
    """4096 -> 64 -> 1024 -> 64 KiB pieces with no release in between: the lanes' blocks are a piece long, so mgXferPrepareLocked drops
    them and they are made again, larger and smaller.  Then 16 threads after 2: the lanes grow.  A round trip of several pieces after
    every change."""
    X = probe()
    n = 2 * DEFAULT_PIECE + P + 7
    data = np.random.default_rng(11).integers(0, 256, n, dtype=np.uint8)
    dev = DevArea(n)
    mg.lib().mgReleaseBuffers()
    try:
        for kb, t in ((4096, 2), (64, 2), (1024, 2), (64, 2), (64, 16), (64, 2)):
            with team(t, kb, release=False):
                what = ("%d KiB pieces" % kb, "T %d" % t)
                upload(X, dev, data, n, 1, 16, t, kb << 10, what + ("H2D",))
                download(X, dev, data, n, 1, 16, t, kb << 10, what + ("D2H",))
    finally:
        mg.lib().mgReleaseBuffers()
    dev.free()


# ---- the saturating add ---------------------------------------------------------------------------

def satadd_inputs(rng, n):
    """host depths and device counts, uniform (about half of the sums saturate), with 0, 1, 65534 and 65535 meeting each other and, at
    every piece edge, sums of exactly 65535 and exactly 65536 on the last element of a piece and the first of the next, alternately"""
    dst = rng.integers(0, 65536, n).astype(np.uint16)
    src = rng.integers(0, 65536, n).astype(np.uint16)
    per = P // 2
    edges = np.arange(per, n, per)
    if n >= 64:
        special = np.array([0, 1, 65534, 65535], np.uint16)
        free = np.setdiff1d(np.arange(n), np.concatenate([edges, edges - 1]))
        at = rng.choice(free, 16, replace=False)
        dst[at] = np.repeat(special, 4); src[at] = np.tile(special, 4)
    for j, e in enumerate(edges):
        lo, hi = (65535, 65536) if j % 2 == 0 else (65536, 65535)
        a = int(rng.integers(1, 65536)); dst[e - 1] = a; src[e - 1] = lo - a
        a = int(rng.integers(1, 65536)); dst[e] = a; src[e] = hi - a
    return dst, src


def run_satadd(X, dev, dst0, src, t, what):
    n = len(src)
    want = np.minimum(dst0.astype(np.uint32) + src, 65535).astype(np.uint16)
    want2 = np.minimum(want.astype(np.uint32) + src, 65535).astype(np.uint16)
    dev.set(2 * n, 0, src.view(np.uint8))
    dst = HostArea(2 * n, 2, dst0.view(np.uint8))        # depth + 1: 2-byte aligned, not 4-byte aligned
    assert dst.addr % 4 == 2
    got = dst.view.view(np.uint16)
    for fold, w in (("first fold", want), ("second fold", want2)):
        before = util.xfer_diag()
        rc = X.xferProbeD2H(dst.addr, dev.addr, 2 * n, MG_XFER_SATADD16)
        after = util.xfer_diag()
        assert rc == 0, what + (fold, mg.lib().mgLastError())
        if not np.array_equal(got, w):
            bad = np.flatnonzero(got != w)
            raise AssertionError(what + (fold, "%d wrong, first at element %d (piece %d, element %d of it): %d, not %d"
                                         % (len(bad), bad[0], bad[0] // (P // 2), bad[0] % (P // 2), int(got[bad[0]]), int(w[bad[0]]))))
        assert dst.fences_intact(), what + (fold, "host bytes outside depth[] were written")
        census_of_one(before, after, 2 * n, t, P, what + (fold,))
    back, fences = dev.read()
    assert fences and np.array_equal(back, src.view(np.uint8)), what + ("the device counts were changed",)


@pytest.mark.parametrize("t", [1, 3, 4])
def test_saturating_add(t):
    """MG_XFER_SATADD16: depth[i] = min (65535, depth[i] + pending[i]) against numpy in 32 bits, one element, around one piece of elements
    and over 3T pieces and a bit; a second fold of the same counts onto the result matches too"""
    X = probe()
    per = P // 2
    lengths = [1, per - 1, per, per + 1, 3 * t * per + 7]
    dev = DevArea(2 * max(lengths), 0)
    rng = np.random.default_rng(16 + t)
    with team(t, 64):
        for d, s in ((65535, 1), (65534, 1), (0, 0), (65535, 65535), (32768, 32768), (32767, 32768)):
            run_satadd(X, dev, np.array([d], np.uint16), np.array([s], np.uint16), t, ("T %d" % t, "one element: %d + %d" % (d, s)))
        for n in lengths:
            dst0, src = satadd_inputs(rng, n)
            if n > per:
                sums = dst0.astype(np.uint32) + src
                assert {int(sums[per - 1]), int(sums[per])} == {65535, 65536}
            run_satadd(X, dev, dst0, src, t, ("T %d" % t, "%d elements" % n))
    dev.free()


# ---- two host threads at once -----------------------------------------------------------------------

def test_two_host_threads_share_the_team():
    """two threads of the caller's (ctypes releases the interpreter's lock during a call) each make 20 round trips of arrays of their own
    on the one device: the team serves one transfer at a time, every result is exact and the census counts them all"""
    X = probe()
    trips = 20
    errors = []

    def work(seed, n):
        try:
            data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
            dev = DevArea(n)
            for i in range(trips):
                src = HostArea(n, seed & 1, np.roll(data, i))
                dev.set(n, 1)
                assert X.xferProbeH2D(dev.addr, src.addr, n) == 0
                got, fences = dev.read()
                assert fences and np.array_equal(got, src.view), (seed, i, "H2D")
                dst = HostArea(n, 1)
                assert X.xferProbeD2H(dst.addr, dev.addr, n, MG_XFER_COPY) == 0
                assert dst.fences_intact() and np.array_equal(dst.view, src.view), (seed, i, "D2H")
            dev.free()
        except BaseException as e:                       # (an assertion in a thread is lost otherwise)
            errors.append(e)

    lengths = (7 * P + 3, 5 * P + P // 2)
    with team(3, 64):
        before = util.xfer_diag()
        th = [threading.Thread(target=work, args=(40 + i, n)) for i, n in enumerate(lengths)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        after = util.xfer_diag()
    assert not errors, errors
    assert after["transfers"] - before["transfers"] == 2 * 2 * trips
    assert after["pieces"] - before["pieces"] == 2 * trips * sum(-(-n // P) for n in lengths)


# ---- the sparse upload ------------------------------------------------------------------------------

SPARSE_BYTES = (6 << 20) + 5000
SPARSE_PAGES = -(-SPARSE_BYTES // PAGE)


def mapped(addr, size):
    """the mapping as an array (making it touches no page)"""
    return np.ctypeslib.as_array((C.c_uint8 * size).from_address(addr))


def present_pages(X, addr, nbytes):
    """(a byte a page of [addr, addr + nbytes): 1 where the page exists, how many do) or (None, -1): /proc/self/pagemap cannot be read"""
    n = (addr + nbytes - 1) // PAGE - addr // PAGE + 1
    bitmap = np.zeros(n, np.uint8)
    count = X.xferProbePresentPages(addr, nbytes, bitmap.ctypes.data)
    assert count == -1 or count == int(bitmap.sum())
    return (bitmap, count) if count >= 0 else (None, -1)


def alternating_runs():
    """written 1, not 2, written 17, not 1, written 2, not 17, ... pages over the whole array"""
    runs, at, i = [], 0, 0
    while at < SPARSE_PAGES:
        ln = (1, 2, 17)[i % 3]
        if i % 2 == 0:
            runs.append((at * PAGE, min((at + ln) * PAGE, SPARSE_BYTES)))
        at += ln; i += 1
    return runs


# name: (offset of hostSrc in the mapping, byte ranges of the mapping that are written, pages that are only read, pages asked to be
# swapped out after they were written, piece KiB, threads)
SPARSE_CASES = {
    "nothing written": (0, [], [], [], None, None),
    "everything written": (0, [(0, SPARSE_BYTES)], [], [], None, None),
    "only the first page": (0, [(0, PAGE)], [], [], None, None),
    "only the last, partial page": (0, [((SPARSE_PAGES - 1) * PAGE, SPARSE_BYTES)], [], [], None, None),
    "alternating runs of 1, 2 and 17 pages": (0, alternating_runs(), [], [], None, None),
    "a run across piece edges, 64 KiB pieces": (0, [(10 * PAGE, 41 * PAGE), (700 * PAGE + 5, 700 * PAGE + 6)], [], [], 64, 3),
    "hostSrc 16 bytes in, its first page written": (16, [(16, PAGE), (5 * PAGE, 7 * PAGE)], [], [], None, None),
    "hostSrc 16 bytes in, its first page not written": (16, [(PAGE, 3 * PAGE)], [], [], None, None),
    "a page that was only read": (0, [(8 * PAGE, 9 * PAGE)], [3, 1200], [], None, None),
    "written pages asked to be swapped out": (0, [(20 * PAGE, 24 * PAGE)], [], [21, 22], None, None),
}


@pytest.mark.parametrize("name", list(SPARSE_CASES))
def test_sparse_upload(name):
    """mgXferH2DSparse of 6 MiB + 5000 bytes of an untouched private anonymous mapping into a device array full of 0xAB: what arrives is
    the host's bytes (read only afterwards), zeros included; the pages that exist are taken from /proc/self/pagemap BEFORE the call, and
    after it the same pages exist and no more (a copy that reads a page makes it exist: tests/test_abi.py shows that on the CPU), the
    census says the page map was used, with as many runs as the bitmap has and the bytes of the other pages not sent"""
    X = probe()
    off, writes, reads, swap_out, kb, t = SPARSE_CASES[name]
    rng = np.random.default_rng(len(name))
    base = X.xferProbeMapAnon(SPARSE_BYTES)
    assert base
    dev = DevArea(SPARSE_BYTES, 0)
    try:
        host = mapped(base, SPARSE_BYTES)
        for lo, hi in writes:
            host[lo:hi] = rng.integers(1, 256, hi - lo, dtype=np.uint8)
        for p in reads:
            assert int(host[p * PAGE + 7]) == 0
        for p in swap_out:
            X.xferProbePageOut(base + p * PAGE, PAGE)
        n = SPARSE_BYTES - off
        dev.set(n, 0, 0xAB)
        with team(t, kb):
            bitmap, count = present_pages(X, base + off, n)
            before = util.xfer_diag()
            rc = X.xferProbeH2DSparse(dev.addr, base + off, n)
            after = util.xfer_diag()
            bitmap2, count2 = present_pages(X, base + off, n)
        assert rc == 0, (name, mg.lib().mgLastError())
        if bitmap is None:
            print("%s: /proc/self/pagemap cannot be read here: the pages that exist and the route taken are not checked" % name)
        else:
            runs = int(bitmap[0]) + int(np.sum((bitmap[1:] == 1) & (bitmap[:-1] == 0)))
            first = (base + off) // PAGE * PAGE
            lo = np.maximum(first + np.arange(len(bitmap)) * PAGE, base + off)
            hi = np.minimum(first + (np.arange(len(bitmap)) + 1) * PAGE, base + off + n)
            sent = int(((hi - lo) * bitmap).sum())
            print("%s: %d of %d pages exist, in %d runs; %d bytes to send" % (name, count, len(bitmap), runs, sent))
            assert count2 == count and np.array_equal(bitmap2, bitmap), (name, "the upload made %d pages exist" % (count2 - count))
            assert after["sparse_by_pagemap"] == before["sparse_by_pagemap"] + 1 and after["sparse_plain"] == before["sparse_plain"], (name, before, after)
            assert after["sparse_runs"] == runs and after["sparse_skipped"] == n - sent, (name, after, runs, n - sent)
            assert after["transfers"] == before["transfers"] + runs, (name, before, after)
            if writes and not swap_out:
                assert count >= sum((hi - 1) // PAGE - lo // PAGE + 1 for lo, hi in writes) // 2      # (the bitmap sees what was written)
        got, fences = dev.read()
        want = host[off:].copy()                         # only now is the host range read
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError((name, "%d wrong, first at byte %d (page %d of the range): %#x, not %#x"
                                  % (len(bad), bad[0], (base + off + bad[0]) // PAGE - (base + off) // PAGE, int(got[bad[0]]), int(want[bad[0]]))))
        assert fences, (name, "device bytes outside the destination were written")
        for lo, hi in writes:
            assert np.all(want[max(lo - off, 0):hi - off] != 0)
    finally:
        dev.free()
        X.xferProbeUnmap(base, SPARSE_BYTES)


@pytest.mark.parametrize("kind", ["one byte under 4 MiB", "a private file mapping", "a shared anonymous mapping", "half anonymous, half a file"])
def test_sparse_upload_takes_the_plain_copy(kind):
    """ranges for which "the page does not exist" does not mean "it reads as zero", and one below the size at which the page map is
    looked at: they take the plain copy (the census says so) and arrive whole.  The file's pages have contents that this process has
    never read."""
    X = probe()
    rng = np.random.default_rng(len(kind))
    n = SPARSE_FLOOR - 1 if kind == "one byte under 4 MiB" else SPARSE_BYTES
    base = {"one byte under 4 MiB": lambda: X.xferProbeMapAnon(n), "a private file mapping": lambda: X.xferProbeMapFile(n, 5),
            "a shared anonymous mapping": lambda: X.xferProbeMapShared(n), "half anonymous, half a file": lambda: X.xferProbeMapHalfFile(n, 6)}[kind]()
    assert base, kind
    dev = DevArea(n, 0)
    try:
        host = mapped(base, n)
        if kind != "a private file mapping":             # some pages written in front, the rest never touched
            for lo, hi in ((0, 3 * PAGE), (40 * PAGE + 9, 57 * PAGE)):
                host[lo:hi] = rng.integers(1, 256, hi - lo, dtype=np.uint8)
        dev.set(n, 0, 0xAB)
        with team(3, 64):
            before = util.xfer_diag()
            rc = X.xferProbeH2DSparse(dev.addr, base, n)
            after = util.xfer_diag()
        assert rc == 0, (kind, mg.lib().mgLastError())
        assert after["sparse_plain"] == before["sparse_plain"] + 1 and after["sparse_by_pagemap"] == before["sparse_by_pagemap"], (kind, before, after)
        assert after["transfers"] == before["transfers"] + 1 and after["pieces"] == before["pieces"] + -(-n // P) and after["threads"] == 3, (kind, before, after)
        got, fences = dev.read()
        want = host.copy()
        if not np.array_equal(got, want):
            raise AssertionError((kind, first_difference(got, want)))
        assert fences, kind
        if kind == "a private file mapping":
            assert np.all(want != 0)
        if kind == "half anonymous, half a file":
            half = -(-(n // 2) // PAGE) * PAGE
            assert np.all(want[half:] != 0) and not np.any(want[3 * PAGE:40 * PAGE])
    finally:
        dev.free()
        X.xferProbeUnmap(base, n)


# ---- the real callers at small pieces ---------------------------------------------------------------

def test_modset_sync_in_small_pieces():
    """a set of 2 * 10^5 entries mirrored with 64 KiB pieces on three lanes: value[] in 25 pieces, depth[] in 7, index[] in 256, against
    the oracle.  Then a second batch, whose counts are pending on the device when the sync comes: modsetSyncToHost folds them into the
    host's depth[] with MG_XFER_SATADD16 over those 7 pieces, and the k-mer of the poly-A read goes past 65535."""
    import test_gpu_modset as tgm
    from oracle import pyoracle as po
    from modimizer_amd import synth
    k, w, bits = 21, 1, 22
    sh = mg.seqhashCreate(k, w, 17); oh = po.Hasher(k, w, 17)
    poly = np.zeros(40_000, np.uint8)
    b1 = util.concat_reads([synth.iid_bases(100_000, 5), poly, synth.iid_bases(100_000, 6)])
    b2 = util.concat_reads([poly, b1[0][30_000:170_000], synth.iid_bases(3_000, 7), b1[0][:60_000]])
    ms = mg.modsetCreate(sh, bits)
    with team(3, 64):
        d0 = util.xfer_diag()
        mg.add_sequence_batch(ms, *b1)
        oms, _ = tgm.oracle_build(oh, bits, [b1])
        assert 190_000 < oms.max < 210_000
        tgm.assert_same_modset(ms, oms, bits)
        d1 = util.xfer_diag()
        print("first sync", d0, d1)
        assert d1["threads"] == 3 and d1["piece_bytes"] == P                    # index[], the last array of the sync
        assert d1["pieces"] - d0["pieces"] >= -(-oms.max * 8 // P) + -(-oms.max * 2 // P) + (4 << bits) // P
        mg.add_sequence_batch(ms, *b2)
        oms2, _ = tgm.oracle_build(oh, bits, [b1, b2])
        assert oms2.depths().max() == 65535 and int(oms.depths().max()) + int(oms.depths().max()) > 65535 > oms.depths().max()
        assert oms2.max > oms.max
        tgm.assert_same_modset(ms, oms2, bits)
        d2 = util.xfer_diag()
        print("second sync", d2)
        assert d2["threads"] == 3 and d2["pieces"] - d1["pieces"] >= -(-oms.max * 2 // P) + (4 << bits) // P
    mg.lib().modsetDestroy(ms)


class CountingLib:
    """the library, with the census taken around every mgReferenceRead"""

    def __init__(self, L):
        self.L, self.census = L, []

    def __getattr__(self, name):
        return getattr(self.L, name)

    def mgReferenceRead(self, *args):
        before = util.xfer_diag()
        rc = self.L.mgReferenceRead(*args)
        self.census.append((before, util.xfer_diag()))
        return rc


def test_reference_mirror_in_small_pieces(tmp_path):
    """one parameter set of the randomized modmap test (tests/test_gpu_modset.py: the seven arrays of mgReferenceRead's mirror and the
    queries, against the oracle) with 64 KiB pieces on three lanes; the padded references have more than 130 000 modimizers, so every
    array of the mirror is several pieces long"""
    import test_gpu_modset as tgm
    k, w, seed = 15, 8, 17
    L = CountingLib(mg.lib())
    with team(3, 64):
        with mg.knobs(FIND_PATH="2 levels", **tgm.TWO_LEVELS):
            tgm._modmap_randomized(L, k, w, seed, tmp_path, pad=130_000 * w)
    assert len(L.census) == 6
    for before, after in L.census:
        print("mgReferenceRead", before, after)
        assert after["threads"] == 3 and after["piece_bytes"] == P, (before, after)      # rev[], the last array of the mirror
        assert after["transfers"] - before["transfers"] >= 7 and after["pieces"] - before["pieces"] >= 6 * 8, (before, after)      # (info[] is a byte an entry: 2 pieces)
