"""modimizer_amd/csrc/mg_prefix.h as primitives: the wave, workgroup and group scans and reductions, driven through the probe library
(oracle/prefix_probe.hip -> oracle/libprefixprobe.so) and held against numpy.  The library's own kernels reach the header only with what
their data happens to be; here the inputs are the edges: sums that wrap in 32 and in 64 bits, carries across bit 32, values that differ
in the high word only, a maximum in lane 0 / 15 / 16 / 31 / 32 / 63, a carry into a max, n around the multiples of the 1024 threads
of mgGroupScan.  Everything is integer arithmetic and numpy wraps as the hardware does: every comparison is exact.

BLOCK_INSTANTIATIONS is plain data (no GPU, no library needed to import this module): tests/test_abi.py asserts that every
mgBlock*<THREADS, Op> the library's kernels use is in it."""
import ctypes as C
import os

import numpy as np
import pytest

import modimizer_amd as mg
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
PROBE_PATH = os.path.join(ORACLE, "libprefixprobe.so")

OPS = {"sum": "MgSum", "max": "MgMax"}
DTYPES = {32: np.uint32, 64: np.uint64}
# what prefixProbeBlock instantiates and test_block_primitives drives: (THREADS, op, bits of T)
BLOCK_INSTANTIATIONS = [(t, op, bits) for t in (64, 256, 1024) for op in OPS for bits in (32, 64)]
GROUPS, PLANES = 3, 6             # prefix_probe.hip: PROBE_GROUPS, PROBE_PLANES

# mgGroupScan<Op, TI, TO, N> as prefixProbeGroup names them: (name, op, bits of TI, bits of TO); "kernel_*" is mgGroupSumKernel<TI, TO> itself
GROUP_INSTANTIATIONS = [("sum_32_32_n32", "sum", 32, 32), ("sum_32_64_n32", "sum", 32, 64), ("sum_32_64_n64", "sum", 32, 64),
                        ("sum_64_64_n32", "sum", 64, 64), ("sum_64_64_n64", "sum", 64, 64), ("max_32_32_n32", "max", 32, 32),
                        ("max_64_64_n64", "max", 64, 64),
                        ("kernel_32_32", "sum", 32, 32), ("kernel_32_64", "sum", 32, 64), ("kernel_64_64", "sum", 64, 64)]
GROUP_LENGTHS = [0, 1, 2, 63, 64, 1023, 1024, 1025, 1536, 2047, 2048, 2049, 3071, 3073, 5000, (1 << 20) + 1]
GUARD = 8


def block_pairs():
    """the (THREADS, Op) pairs of BLOCK_INSTANTIATIONS as the kernels spell them"""
    return {(t, OPS[op]) for t, op, _ in BLOCK_INSTANTIATIONS}


# ---- the probe ----------------------------------------------------------------------------------

PROBE_SOURCES = ["prefix_probe.hip", "../modimizer_amd/csrc/mg_prefix.h"]
PROBE_MARKER = "PREFIX_PROBE_HASH"


def probe_source_hash():
    """the hash oracle/Makefile bakes into the probe, over its two sources"""
    return util.probe_source_hash(PROBE_SOURCES)


def probe_binary_hash(path=None):
    """the hash a built probe carries, read out of the file (no dlopen); None if there is no such file or marker"""
    return util.probe_binary_hash(path or PROBE_PATH, PROBE_MARKER)


def build_probe():
    """make the probe if the one in the tree is not the build of the tree's sources"""
    return util.build_probe("libprefixprobe.so", PROBE_MARKER, PROBE_SOURCES)


_probe = None


def probe():
    global _probe
    if _probe is None:
        mg.lib()                                         # first: one HIP runtime in the process
        P = C.CDLL(build_probe())
        P.prefixProbeHash.restype = C.c_char_p
        if P.prefixProbeHash().decode() != probe_source_hash():
            raise RuntimeError("libprefixprobe.so (%s) is not the build of this tree's prefix_probe.hip and mg_prefix.h (%s)"
                               % (P.prefixProbeHash().decode(), probe_source_hash()))
        P.prefixProbeBlock.restype = C.c_int
        P.prefixProbeBlock.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
        P.prefixProbeGroup.restype = C.c_int
        P.prefixProbeGroup.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        _probe = P
    return _probe


@pytest.mark.gpu
def test_probe_is_the_build_of_this_tree():
    P = probe()
    assert P.prefixProbeHash().decode() == probe_source_hash() == probe_binary_hash()
    # what it does not instantiate is refused, not run as something else
    v = np.zeros(GROUPS * 1024, np.uint64); out = np.zeros(PLANES * GROUPS * 1024, np.uint64); ret = C.c_uint64(0)
    assert P.prefixProbeBlock(512, b"sum", 32, v.ctypes.data, out.ctypes.data) == -1
    assert P.prefixProbeBlock(256, b"min", 32, v.ctypes.data, out.ctypes.data) == -1
    assert P.prefixProbeGroup(b"max_32_64_n32", v.ctypes.data, out.ctypes.data, 4, 0, 0, 0, C.byref(ret)) == -1
    assert P.prefixProbeGroup(b"sum_32_64_n32", v.ctypes.data, out.ctypes.data, 4, 0, 0, 1, C.byref(ret)) == -1      # in place needs one width


# ---- references -----------------------------------------------------------------------------------

def scan(op, x, axis=-1):
    """inclusive scan in x's own unsigned type: the sum wraps as the hardware's does"""
    return np.cumsum(x, axis=axis, dtype=x.dtype) if op == "sum" else np.maximum.accumulate(x, axis=axis)


def combine(op, a, b):
    return (a + b).astype(b.dtype) if op == "sum" else np.maximum(a, b)


def shifted(inc):
    """the exclusive values from the inclusive ones: 0, the identity of both operations, in front"""
    return np.concatenate([np.zeros(1, inc.dtype), inc[:-1]])


def block_reference(op, v):
    """the six planes of probeBlockKernel for ONE workgroup's values v"""
    inc = scan(op, v)
    total = np.full_like(v, inc[-1])
    waves = v.reshape(-1, 64)
    w_inc = scan(op, waves, axis=1)
    w_red = np.repeat(w_inc[:, -1], 64)
    return [inc, total, shifted(inc), total, w_inc.reshape(-1), w_red]


def block_inputs(threads, op, bits):
    """(name, values of one workgroup) for an instantiation"""
    dt = DTYPES[bits]
    rng = np.random.default_rng(1000 * threads + 10 * bits + (op == "max"))
    top = (1 << bits) - 1
    big = dt(0x80000001) if bits == 32 else dt(0x8000000100000003)
    full = lambda: rng.integers(0, top, threads, dtype=dt, endpoint=True)
    cases = [("zeros", np.zeros(threads, dt)), ("ones", np.ones(threads, dt)), ("arange", np.arange(threads, dtype=dt)),
             ("random, full width", full()), ("random, full width, again", full()),         # U32 sums wrap; U64 sums pass 2^32 and 2^64
             ("random, small", rng.integers(0, 1000, threads).astype(dt))]
    for p in (0, 15, 16, 31, 32, 63, 64, threads - 1):
        if p < threads:
            v = np.zeros(threads, dt); v[p] = big
            cases.append(("one value at %d" % p, v))
            v = rng.integers(1, 1000, threads).astype(dt); v[p] = big                       # the maximum sits there, the others are not 0
            cases.append(("the maximum at %d" % p, v))
    asc = np.sort(rng.choice(1 << 20, threads, replace=False)).astype(dt) + dt(1)
    ties = np.repeat(rng.integers(1, 1 << 30, (threads + 36) // 37).astype(dt), 37)[:threads]
    cases += [("ascending", asc), ("descending", asc[::-1].copy()), ("runs of ties", ties), ("all equal, top value", np.full(threads, top, dt))]
    if bits == 64:
        lo, hi = np.uint64(0xFFFFFFFF), np.uint64(1 << 32)
        alt = np.where(np.arange(threads) % 2 == 0, hi, lo).astype(dt)
        cases += [("every value 0xFFFFFFFF", np.full(threads, lo, dt)),                      # every add carries into the high word
                  ("1 << 32 and 0xFFFFFFFF alternating", alt),                                # a max over one word only fails on one of the two
                  ("0xFFFFFFFF and 1 << 32 alternating", np.where(np.arange(threads) % 2 == 0, lo, hi).astype(dt)),
                  ("high words differ, low words equal", (rng.integers(0, 1 << 31, threads).astype(dt) << dt(32)) | dt(0x12345678)),
                  ("high words equal, low words differ", (dt(7) << dt(32)) | rng.integers(0, 1 << 32, threads).astype(dt))]
    return cases


PLANE_NAMES = ["mgBlockInclusive", "mgBlockInclusive's total", "mgBlockExclusive", "mgBlockReduce", "mgWaveInclusive", "mgWaveReduce"]


@pytest.mark.gpu
@pytest.mark.parametrize("threads,op,bits", BLOCK_INSTANTIATIONS)
def test_block_primitives(threads, op, bits):
    """the five calls back to back on one lds array, three workgroups with different inputs per launch"""
    P = probe()
    dt = DTYPES[bits]
    cases = block_inputs(threads, op, bits)
    while len(cases) % GROUPS:
        cases.append(("zeros, to fill the grid", np.zeros(threads, dt)))
    n = GROUPS * threads
    for at in range(0, len(cases), GROUPS):
        v = np.concatenate([c[1] for c in cases[at:at + GROUPS]])
        assert v.dtype == dt and len(v) == n
        out = np.zeros(PLANES * n, dt)
        assert P.prefixProbeBlock(threads, op.encode(), bits, v.ctypes.data, out.ctypes.data) == 0
        out = out.reshape(PLANES, GROUPS, threads)
        for g in range(GROUPS):
            name, x = cases[at + g]
            for plane, want in enumerate(block_reference(op, x)):
                got = out[plane, g]
                bad = np.flatnonzero(got != want)
                assert np.array_equal(got, want), (PLANE_NAMES[plane], name, "workgroup %d" % g, "first at thread %d: %#x, not %#x"
                                                   % (bad[0], int(got[bad[0]]), int(want[bad[0]])))


# ---- mgGroupScan ------------------------------------------------------------------------------------

def group_inputs(op, bits_in, n, rng):
    dt = DTYPES[bits_in]
    if op == "sum":                                  # full width: a U32 sum wraps, a U32 -> U64 sum passes 2^32, a U64 sum wraps
        return rng.integers(0, (1 << bits_in) - 1, n, dtype=dt, endpoint=True)
    if bits_in == 32:                                # a band with room below and above for the carries
        return rng.integers(1 << 10, 1 << 31, n).astype(dt)
    return (rng.integers(2, 1 << 30, n).astype(dt) << dt(32)) | rng.integers(0, 1 << 32, n).astype(dt)


def group_carries(op, bits_out, x):
    if op == "sum":
        return [0, 0xFFFFFFF0]                       # with any input at all the sum passes 2^32: it wraps in a U32 and carries into the high word of a U64
    if len(x) == 0:
        return [0, 12345]
    srt = np.sort(x)
    return [0, int(srt[-1]) + 1, int(srt[len(x) // 2]), int(srt[0]) - 1]      # none; above every input; between them; below every input


def run_group(name, op, bits_in, bits_out, x, carry, in_place):
    """one probe call; asserts everything that is to hold of it"""
    P = probe()
    ti, to = DTYPES[bits_in], DTYPES[bits_out]
    n = len(x)
    inc = scan(op, x.astype(to))
    c = np.array([carry], to)
    want = combine(op, c, shifted(inc)[:n]) if n else np.zeros(0, to)
    want_ret = int(combine(op, c, inc[-1:])[0]) if n else carry
    fence = to(0xDEADBEEFDEADBEEF & ((1 << bits_out) - 1))
    buf = np.full(n + 2 * GUARD, fence, to)
    buf[GUARD:GUARD + n] = x if in_place else to(0x5A5A5A5A)
    before = buf.copy()
    xin = x.copy()
    ret = C.c_uint64(0)
    what = (name, "n %d" % n, "carry %#x" % carry, "in place" if in_place else "distinct buffers")
    assert P.prefixProbeGroup(name.encode(), xin.ctypes.data, buf.ctypes.data, n, carry, GUARD, int(in_place), C.byref(ret)) == 0, what
    assert ret.value == want_ret, what + ("returned %#x, not %#x" % (ret.value, want_ret),)
    got = buf[GUARD:GUARD + n]
    bad = np.flatnonzero(got != want)
    assert np.array_equal(got, want), what + ("first at %d: %#x, not %#x" % (bad[0], int(got[bad[0]]), int(want[bad[0]])),)
    assert np.array_equal(buf[:GUARD], before[:GUARD]) and np.array_equal(buf[GUARD + n:], before[GUARD + n:]), what + ("words outside out[0 .. n) were written",)
    assert np.array_equal(xin, x), what + ("in[] was changed",)
    if n == 0:
        assert np.array_equal(buf, before), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", GROUP_LENGTHS)
@pytest.mark.parametrize("name,op,bits_in,bits_out", GROUP_INSTANTIATIONS)
def test_group_scan(name, op, bits_in, bits_out, n):
    """out[i] = carryIn op in[0] op ... op in[i - 1], the return value in a word of its own, nothing else written: distinct buffers
    and (one width) in place, every carry"""
    rng = np.random.default_rng(n * 131 + bits_in + 7 * bits_out + (op == "max"))
    x = group_inputs(op, bits_in, n, rng)
    carries = [0] if name.startswith("kernel") else group_carries(op, bits_out, x)
    for carry in carries:
        for in_place in ([False, True] if bits_in == bits_out else [False]):
            run_group(name, op, bits_in, bits_out, x, carry, in_place)


@pytest.mark.gpu
@pytest.mark.parametrize("name,op,bits_in,bits_out", GROUP_INSTANTIATIONS)
def test_group_scan_sparse_counts(name, op, bits_in, bits_out):
    """tile counts as the kernels have them: mostly 0, so most threads' pieces hold nothing and the value at a thread boundary is one
    that came from far away"""
    rng = np.random.default_rng(5 + bits_in + bits_out)
    for n in (1025, 2049, 5000):
        x = np.zeros(n, DTYPES[bits_in])
        at = rng.choice(n, 7, replace=False)
        x[at] = group_inputs(op, bits_in, 7, rng)
        x[0] = 0                                          # (the first piece empty too)
        for carry in ([0] if name.startswith("kernel") else [0, 0xFFFFFFF0 if op == "sum" else int(x.max()) // 2]):
            run_group(name, op, bits_in, bits_out, x, carry, bits_in == bits_out)
