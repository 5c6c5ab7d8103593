"""modutils -wt / -rt on the GPU (modutils.c:169-199): mgModsetWriteTextDevice and mgModsetReadText against the reference program's own
files (tests/golden/modutils_*.dump*, text_*: made by make_golden.py / make_golden_text.py), against the host loop mgModsetWriteText,
and at a size past the formatter's chunk of 2^24 lines.  Every read asserts which of the three paths ran (mgModsetReadTextPath):
0 = parsed on the device, 1 = parsed on the host and inserted on the device, 2 = built on the host."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
import util
from test_gpu_report import build_set, device_block

pytestmark = pytest.mark.gpu
TAGS = list(util.MODUTILS_TAGS)


def gpath(name):
    return os.path.join(util.GOLDEN, name)


def host_text(ms, path):
    """mgModsetWriteText: the host loop (it syncs the set first)"""
    with mg.CFile(path, "w") as f:
        mg.lib().mgModsetWriteText(ms, f)
    return open(path).read()


def device_text(ms, path):
    mg.write_text_device(ms, path)
    return open(path).read()


def destroy(ms):
    L = mg.lib()
    sh = C.cast(ms.contents.hasher, C.c_void_p).value              # (the field itself is a view into *ms)
    L.modsetDestroy(ms)
    L.mgSeqhashDestroy(C.cast(sh, C.POINTER(mg.Seqhash)))


def synced_arrays(ms):
    mg.check(mg.lib().modsetSyncToHost(ms, 1))
    return (ms.contents.max,) + mg.modset_arrays(ms)


def same_arrays(a, b):
    """max, value[1 .. max], depth[], info[] (value[0] is no entry: modsetCreate leaves it as malloc gave it)"""
    return a[0] == b[0] and np.array_equal(a[1][1:], b[1][1:]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def index_table(ms):
    return np.ctypeslib.as_array(ms.contents.index, (1 << ms.contents.tableBits,))


def strip_timing(text):
    return "\n".join(l for l in text.splitlines() if not l.startswith("user\t") and "resources used" not in l
                     and not l.startswith("total resources")) + "\n"


# ---- 1: -wt against the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["pending", "synced", "loaded"])
@pytest.mark.parametrize("tag", TAGS)
def test_write_text_device_matches_reference(tag, state, tmp_path):
    L = mg.lib()
    ms = build_set(tag, state, tmp_path)
    mx = ms.contents.max
    text = device_text(ms, str(tmp_path / "dev.txt"))
    util.check_dump(text, "modutils_%s.dump.txt" % tag)
    assert ms.contents.max == mx
    assert text == host_text(ms, str(tmp_path / "host.txt"))
    # the set is what it was: the same bytes again, and the host arrays once synced do not move
    before = synced_arrays(ms)
    assert device_text(ms, str(tmp_path / "dev2.txt")) == text
    assert same_arrays(before, synced_arrays(ms))
    L.modsetDepthPrune(ms, 2, 40)
    pruned = device_text(ms, str(tmp_path / "pruned.txt"))
    util.check_dump(pruned, "modutils_%s.pruned_dump.txt" % tag)
    assert pruned == host_text(ms, str(tmp_path / "pruned_host.txt"))
    L.modsetDestroy(ms)

    if tag == "k21d64" and state == "pending":
        # examples/text_file.c: modutils -rt dump -p 2 40 -wt out
        exe = str(tmp_path / "text_file")
        libdir = os.path.join(util.ROOT, "modimizer_amd")
        r = subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"),
                            os.path.join(util.ROOT, "examples", "text_file.c"), "-o", exe, "-L", libdir, "-lmodgpu",
                            "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe, "-rt", str(tmp_path / "dev.txt"), "-p", "2", "40", "-wt", str(tmp_path / "ex.txt")],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-800:]
        assert open(tmp_path / "ex.txt").read() == pruned
        want = util.golden_text("text_%s.rt.stdout.txt" % tag) + "".join(util.golden_text("modutils_%s.stdout.txt" % tag).splitlines(keepends=True)[-3:])
        assert r.stdout == want


# ---- 2: -rt round trip against the reference -------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_read_text_round_trip_matches_reference(tag, tmp_path):
    L = mg.lib()
    ms0 = build_set(tag, "pending", tmp_path)
    dump = str(tmp_path / "dump.txt")
    text = device_text(ms0, dump)
    orig = synced_arrays(ms0)
    ms = mg.read_text(dump)
    assert mg.read_text_path() == 0
    assert L.mgModsetDeviceSlots(ms) > 0
    assert ms.contents.max == orig[0]
    assert same_arrays(orig, synced_arrays(ms))
    assert np.array_equal(index_table(ms), index_table(ms0))
    # modutils_ref -rt dump -w: the .mod bytes, index[] included
    p = str(tmp_path / "rt.mod")
    with mg.CFile(p, "w") as f:
        L.modsetWrite(ms, f)
    assert open(p, "rb").read() == gzip.open(gpath("text_%s.rt.mod" % tag)).read()
    with mg.CFile(str(tmp_path / "summary.txt"), "w") as f:
        L.modsetSummary(ms, f)
    assert strip_timing(open(tmp_path / "summary.txt").read()) == util.golden_text("text_%s.rt.stdout.txt" % tag)
    # and as text again
    assert device_text(ms, str(tmp_path / "again.txt")) == text
    destroy(ms)
    L.modsetDestroy(ms0)


# ---- 3 - 5: hand-written tables ----------------------------------------------------------------------------------------------

def test_duplicates_and_letters_on_the_device_path(tmp_path):
    """text_dups.txt, strict grammar: a k-mer in lower and in upper case with different depths, tokens of n and of a (both value 0),
    a byte that is no letter, depth 70000 and info 300 (truncated to 16 and 8 bits), a negative index.  The last line of a k-mer gives
    its values, its first line its place: 7 lines, 5 entries."""
    ms = mg.read_text(gpath("text_dups.txt"))
    assert mg.read_text_path() == 0
    assert ms.contents.max == 5 and ms.contents.size == 8
    want = util.golden_text("text_dups.dump.txt")
    assert device_text(ms, str(tmp_path / "d.txt")) == want
    assert host_text(ms, str(tmp_path / "h.txt")) == want
    destroy(ms)


def test_tail_behind_the_last_wanted_line_and_missing_final_newline(tmp_path):
    """what follows the size - 1-th line is not looked at (the device path stays the device path); a last line without its newline, or
    lines that end in CR LF, are the host parser's, with the same set"""
    text = util.golden_text("text_dups.txt")
    want = util.golden_text("text_dups.dump.txt")
    for name, body, path in (("tail", text + "8 this is not a line\n\n\tx\n", 0), ("open", text[:-1], 1), ("crlf", text.replace("\n", "\r\n"), 1)):
        p = tmp_path / (name + ".txt")
        p.write_bytes(body.encode())
        ms = mg.read_text(str(p))
        assert mg.read_text_path() == path, name
        assert device_text(ms, str(tmp_path / "d.txt")) == want, name
        destroy(ms)


def test_loose_input_takes_the_host_parser(tmp_path):
    """text_loose.txt: blanks for tabs, a leading blank, an empty line, +6, two records on one line, 65541 / 259, lines after the
    size - 1-th: what the reference's fscanf accepts"""
    ms = mg.read_text(gpath("text_loose.txt"))
    assert mg.read_text_path() == 1
    assert mg.lib().mgModsetDeviceSlots(ms) > 0
    want = util.golden_text("text_loose.dump.txt")
    assert device_text(ms, str(tmp_path / "d.txt")) == want
    assert host_text(ms, str(tmp_path / "h.txt")) == want
    destroy(ms)


def test_long_token_builds_the_set_on_the_host(tmp_path):
    """text_long.txt: a token of 32 letters at k = 21 whose value is 4^21 or more: no device table may hold it"""
    L = mg.lib()
    ms = mg.read_text(gpath("text_long.txt"))
    assert mg.read_text_path() == 2
    assert L.mgModsetDeviceSlots(ms) == 0
    assert ms.contents.max == 3 and int(ms.contents.value[2]) >> 42
    assert host_text(ms, str(tmp_path / "h.txt")) == util.golden_text("text_long.dump.txt")
    assert L.mgModsetDeviceSlots(ms) == 0
    with pytest.raises(mg.ModgpuError, match="4\\^k or more"):                 # the device writer refuses such a set
        mg.write_text_device(ms, str(tmp_path / "d.txt"))
    assert L.mgModsetDeviceSlots(ms) == 0
    destroy(ms)


# ---- 6: errors -----------------------------------------------------------------------------------------------------------------

ERROR_CASES = json.load(open(gpath("text_errors.json")))


def device_free_bytes():
    try:
        import torch
        return torch.cuda.mem_get_info()[0]
    except Exception:
        return None


def test_errors_carry_the_reference_text_and_leave_nothing(tmp_path):
    """every case of text_errors.json: 0 and the reference's text after "FATAL ERROR: " (the 40-byte token, which overruns a buffer in
    the reference: the library's own "bad line N").  The cases that reach the device, over and over, do not eat its memory (every
    buffer of a call is released when it returns: the windows alone are 2 MiB a call), and a good file is read right afterwards."""
    L = mg.lib()
    assert [c["name"] for c in ERROR_CASES] == ["depth_not_a_number", "fewer_lines", "bits_19", "size_too_big", "size_negative", "k_32", "w_0",
                                                "missing_file", "mangled_header", "long_token"]
    paths = {}
    for c in ERROR_CASES:
        path = str(tmp_path / ("%s.txt" % c["name"]))
        if c["input"] is not None:
            open(path, "w").write(c["input"])
        paths[c["name"]] = path
        assert not L.mgModsetReadText(path.encode()), c["name"]
        assert L.mgLastError().decode() == c["message"].replace("<FILE>", path), c["name"]
    assert [c["message"] for c in ERROR_CASES[:2]] == ["bad line 3", "bad line 3"] and ERROR_CASES[-1]["message"] == "bad line 2"
    ms = mg.read_text(gpath("text_dups.txt"))
    destroy(ms)
    free0 = device_free_bytes()
    for _ in range(100):
        for name in ("depth_not_a_number", "fewer_lines", "long_token"):
            assert not L.mgModsetReadText(paths[name].encode())
    free1 = device_free_bytes()
    if free0 is not None:
        assert free1 >= free0 - (128 << 20), (free0, free1)
    ms = mg.read_text(gpath("text_dups.txt"))
    assert mg.read_text_path() == 0
    assert device_text(ms, str(tmp_path / "d.txt")) == util.golden_text("text_dups.dump.txt")
    destroy(ms)


# ---- 7: empty sets ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [0, 1])
def test_empty_sets(size, tmp_path):
    L = mg.lib()
    p = tmp_path / "empty.txt"
    p.write_text("modset bits 21 size %d k 19 w 31 seed 5\n" % size)
    ms = mg.read_text(str(p))
    assert mg.read_text_path() == 0
    assert ms.contents.max == 0 and ms.contents.tableBits == 21
    sh = ms.contents.hasher.contents
    assert (sh.k, sh.w, sh.seed) == (19, 31, 5)
    if size == 0:
        other = mg.modsetCreate(mg.seqhashCreate(19, 31, 5), 21, 0)
        assert ms.contents.size == other.contents.size == (1 << 19) - 1
        destroy(other)
    else:
        assert ms.contents.size == 1
    want = "modset bits 21 size 1 k 19 w 31 seed 5\n"
    assert device_text(ms, str(tmp_path / "d.txt")) == want
    assert host_text(ms, str(tmp_path / "h.txt")) == want
    destroy(ms)


# ---- 8: window edges ---------------------------------------------------------------------------------------------------------------

def test_window_edges(tmp_path):
    """MODGPU_TEXT_WINDOW_KB=1 (windows of one 4 KiB tile): the k31d4 dump, whose lines of about 45 bytes straddle every window's end;
    and a table whose lines all have 32 bytes, so that every window ends exactly on a newline"""
    L = mg.lib()
    ms0 = build_set("k31d4", "pending", tmp_path)
    dump = str(tmp_path / "dump.txt")
    device_text(ms0, dump)
    orig = synced_arrays(ms0)
    assert os.path.getsize(dump) > 100 * 4096
    with mg.knobs(TEXT_WINDOW_KB=1):
        ms = mg.read_text(dump)
        assert mg.read_text_path() == 0
        assert same_arrays(orig, synced_arrays(ms))
        assert np.array_equal(index_table(ms), index_table(ms0))
        destroy(ms)
    L.modsetDestroy(ms0)

    rng = np.random.default_rng(11)
    n = 700
    keys = rng.choice(1 << 42, n, replace=False).astype(np.uint64)
    lines, depth, info = [], [], []
    for i in range(1, n + 1):
        room = 32 - 25 - len(str(i))                      # digits of depth and info together
        dd = int(rng.integers(1, room))                   # 1 .. room - 1
        d = int(rng.integers(10 ** (dd - 1), 10 ** dd)); f = int(rng.integers(10 ** (room - dd - 1), 10 ** (room - dd)))
        kmer = "".join("acgt"[(int(keys[i - 1]) >> (2 * b)) & 3] for b in range(20, -1, -1))
        lines.append("%d\t%s\t%d\t%d\n" % (i, kmer, d, f))
        assert len(lines[-1]) == 32
        depth.append(d & 0xffff); info.append(f & 0xff)
    p = tmp_path / "even.txt"
    p.write_text("modset bits 20 size %d k 21 w 64 seed 17\n" % (n + 1) + "".join(lines))
    with mg.knobs(TEXT_WINDOW_KB=1):
        ms = mg.read_text(str(p))
        assert mg.read_text_path() == 0
    mx, v, d, f = synced_arrays(ms)
    assert mx == n and np.array_equal(v[1:], keys) and d[1:].tolist() == depth and f[1:].tolist() == info
    destroy(ms)


# ---- 9: at size ------------------------------------------------------------------------------------------------------------------------

def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def test_round_trip_past_the_formatter_chunk(tmp_path):
    """more than 2^24 + 12345 entries (the formatter takes 2^24 lines a chunk; the reader many windows): a synthetic set built with
    mgAddReadsDevice from mgSynthReads input, info[] set on the host; written by the device and by the host loop (same sha256), read
    back on the device path: value, depth, info and, after modsetSyncToHost (.., 1), index[] equal the original's"""
    L = mg.lib()
    k, w, bits = 21, 16, 27
    d_r, d_of, tot, nr = device_block(L, 520_000_000, 20_000_000, 3000, 779)
    ms0 = mg.modsetCreate(mg.seqhashCreate(k, w, 17), bits)
    n = C.c_uint64()
    mg.check(L.mgAddReadsDevice(ms0, d_r.ptr, tot, d_of.ptr, nr, C.byref(n), None))
    d_r.free(); d_of.free()
    mx = ms0.contents.max
    assert mx >= (1 << 24) + 12345
    mg.check(L.modsetSyncToHost(ms0, 1))
    np.ctypeslib.as_array(ms0.contents.info, (mx + 1,))[1:] = (np.arange(1, mx + 1, dtype=np.uint64) * 7 % 256).astype(np.uint8)
    dev, host = str(tmp_path / "dev.txt"), str(tmp_path / "host.txt")
    mg.write_text_device(ms0, dev)
    with mg.CFile(host, "w") as f:
        L.mgModsetWriteText(ms0, f)
    assert os.path.getsize(dev) == os.path.getsize(host)
    assert sha256_file(dev) == sha256_file(host)
    os.remove(host)
    orig = synced_arrays(ms0)
    assert orig[0] == mx and int(orig[2].max()) > 9
    ms = mg.read_text(dev)
    assert mg.read_text_path() == 0
    assert same_arrays(orig, synced_arrays(ms))
    assert np.array_equal(index_table(ms), index_table(ms0))
    destroy(ms)
    destroy(ms0)
