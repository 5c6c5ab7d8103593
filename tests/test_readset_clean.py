"""modasm -C and -P (cleanMods, modasm.c:514-555; readProperties, modasm.c:912-952): a plain numpy restatement of both passes against the
reference program's own output (tests/golden/clean_*: make_golden_clean.py), which the randomized GPU tests (test_gpu_readset_clean.py) then
lean on; the library's host loops against the same files; the four names in header, library and binding."""
import gzip
import os
import re

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests import test_readset as trs

TAGS = {"k19d8": (19, 8)}
TOPMASK = 0x7fffffff
MS_MINOR, MS_REPEAT, MS_INTERNAL, MS_RDNA = 4, 8, 0x10, 0x20
NAMES = ["mgReadsetCleanMods", "mgReadsetCleanModsPath", "mgReadsetProperties", "mgReadsetPropertiesPath"]


# ---- the restatement: a = test_readset.lib_arrays (reads from 0 here: read i of the reference is row i - 1), depth / info = ms's arrays ----

def clean_mods(a, depth, info, w):
    """(info afterwards, the printed line, nCopy[nReads][4]).  The reference starts its Read pointer at entry 0 while it counts from 1
    (modasm.c:522-523): reads 1 .. nReads - 1 contribute, the last one does not."""
    info = info.copy()
    mod = (a["hit"] & TOPMASK).astype(np.int64)
    dx, hs, n = a["dx"].astype(np.int64), a["hitStart"].astype(np.int64), len(a["nHit"])
    ends = hs[1:]                                                                 # hitStart holds nReads + 1 places
    for r in range(n - 1):
        m, d = mod[hs[r]:ends[r]], dx[hs[r]:ends[r]]
        u, c = np.unique(m, return_counts=True)
        info[u[c >= 2]] |= MS_REPEAT                                             # orientation ignored
        if len(m) >= 3:
            j = np.arange(1, len(m) - 1)
            info[m[j[(d[j] < w) & (d[j + 1] < w)]]] |= MS_INTERNAL
        dp = depth[m].astype(np.int64)                                          # as int: 65535 for a saturated mod
        info[m[1:][dp[:-1] > 2 * dp[1:]]] |= MS_MINOR
        info[m[:-1][dp[1:] > 2 * dp[:-1]]] |= MS_MINOR
    line = "set %d repeated, %d internal, %d minor_variant mods\n" % tuple(int(((info & f) != 0).sum()) for f in (MS_REPEAT, MS_INTERNAL, MS_MINOR))
    ncopy = np.array([np.bincount(info[mod[hs[r]:ends[r]]] & 3, minlength=4) for r in range(n)], np.int64).reshape(n, 4)
    return info, line, ncopy


def read_properties(a, info):
    """the lines of -P: every read, the last included"""
    hit = a["hit"].astype(np.int64)
    hs, n = a["hitStart"].astype(np.int64), len(a["nHit"])
    ends = hs[1:]                                                                 # hitStart holds nReads + 1 places
    out = []
    for r in range(n):
        h = hit[hs[r]:ends[r]]
        h = h[(info[h & TOPMASK] & 3) == 1]
        u, inv = np.unique(h & TOPMASK, return_inverse=True)
        f = np.bincount(inv, weights=(h >> 31) & 1, minlength=len(u)).astype(np.int64)
        rv = np.bincount(inv, minlength=len(u)).astype(np.int64) - f
        t = f + rv
        rev2 = (f == 1) & (rv == 1)
        tan2 = (t == 2) & ~rev2
        more_rev = (t > 2) & (f > 0) & (rv > 0)
        more_tan = (t > 2) & ~more_rev
        out += ["MT i %d h %d count %d\n" % (r + 1, u[q], t[q]) for q in np.flatnonzero(more_tan)]
        out.append("READ %d n %d n2Tan %d n2Rev %d nMoreTan %d nMoreRev %d\n" % (r + 1, len(u), tan2.sum(), rev2.sum(), more_tan.sum(), more_rev.sum()))
        if more_tan.sum() > 5:
            out.append("RM %d nMoreTan %d" % (r + 1, more_tan.sum()) + "".join(" %d" % x for x in u[t > 2]) + "\n")
    return "".join(out)


# ---- helpers shared with the GPU tests ----

def golden_stem(golden_dir, tag):
    return os.path.join(golden_dir, "clean_%s" % tag)


def golden_lines(tag):
    """(the -C line, the -P lines) of `modasm -r clean_<tag> -C -P -w clean_<tag>_C`"""
    text = util.golden_text("clean_%s.stdout.txt" % tag)
    first, rest = text.split("\n", 1)
    assert first.startswith("set ") and rest.startswith("READ ")
    return first + "\n", rest


def ms_arrays(ms):
    _, depth, info = mg.modset_arrays(ms)
    return depth, info


def written_equals_golden(out, stem_c, mod_mask=None):
    """<out>.mod / .readset are the reference's clean_<tag>_C files: the .mod bytes (value[0], which a set made from the source .mod never
    initialises, masked on request), the .readset but for the addresses it holds"""
    got, want = gzip.open(out + ".mod").read(), gzip.open(stem_c + ".mod").read()
    assert (mod_mask(got) == mod_mask(want)) if mod_mask else (got == want)
    assert trs.readset_mask(gzip.open(out + ".readset").read()) == trs.readset_mask(gzip.open(stem_c + ".readset").read())


class host_loops:
    """MODGPU_READSET_HOST=1 around a block: -C and -P by the library's host loops"""
    def __enter__(self):
        os.environ["MODGPU_READSET_HOST"] = "1"; mg.lib().mgReloadKnobs()

    def __exit__(self, *a):
        del os.environ["MODGPU_READSET_HOST"]; mg.lib().mgReloadKnobs()


# ---- the tests ----

@pytest.mark.parametrize("tag", list(TAGS))
def test_restatement_vs_reference_program(tag, golden_dir, tmp_path):
    """the numpy restatement on the reference's own clean_<tag>.mod / .readset: its -C line, the info bytes of the .mod it wrote after -C,
    the nCopy it wrote, its -P lines -- with the last read tandem-duplicated, which -C must not see and -P must"""
    L = mg.lib()
    stem = golden_stem(golden_dir, tag)
    rs = L.mgReadsetLoad(stem.encode())
    a = trs.lib_arrays(rs)
    depth, info = ms_arrays(rs.contents.ms)
    w = rs.contents.ms.contents.hasher.contents.w
    assert w == TAGS[tag][1]
    c_line, p_lines = golden_lines(tag)
    info2, line, ncopy = clean_mods(a, depth, info, w)
    assert line == c_line
    rs_c = L.mgReadsetLoad((stem + "_C").encode())
    depth_c, info_c = ms_arrays(rs_c.contents.ms)
    assert np.array_equal(info2, info_c) and np.array_equal(depth, depth_c)
    assert np.array_equal(ncopy, trs.lib_arrays(rs_c)["nCopy"])
    assert not np.array_equal(info, info_c)
    assert read_properties(a, info) == p_lines == read_properties(a, info2)        # the flags of -C leave the copy classes alone
    # the last read: a restatement that looked at it would set more repeat flags
    n = len(a["nHit"])
    last = (a["hit"][int(a["hitStart"][n - 1]):] & TOPMASK)
    assert len(set(last.tolist())) < len(last) and not (info_c[np.unique(last)] & MS_REPEAT).any()
    for x in (rs, rs_c):
        L.mgReadsetDestroy(x)


@pytest.mark.parametrize("tag", list(TAGS))
def test_host_loops_vs_reference_program(tag, golden_dir, tmp_path):
    """the library's host loops (the path of a set too large for the device), forced by MODGPU_READSET_HOST=1: the reference's lines and files"""
    L = mg.lib()
    stem = golden_stem(golden_dir, tag)
    c_line, p_lines = golden_lines(tag)
    rs = L.mgReadsetLoad(stem.encode())
    info0 = ms_arrays(rs.contents.ms)[1]
    with host_loops():
        assert mg.readset_properties(rs, str(tmp_path / "p.txt")) == 1
        assert open(tmp_path / "p.txt").read() == p_lines and np.array_equal(ms_arrays(rs.contents.ms)[1], info0)
        for again in range(2):                                                    # a second -C changes nothing
            assert mg.readset_clean_mods(rs, str(tmp_path / "c.txt")) == 1
            assert open(tmp_path / "c.txt").read() == c_line
            out = str(tmp_path / ("out%d" % again))
            L.mgReadsetWrite(rs, out.encode())
            written_equals_golden(out, stem + "_C")
        assert mg.readset_properties(rs, str(tmp_path / "p2.txt")) == 1 and open(tmp_path / "p2.txt").read() == p_lines
    L.mgReadsetDestroy(rs)


def test_names_in_header_library_and_binding():
    header = open(os.path.join(util.ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n in NAMES:
        assert re.search(r"^int  %s \(" % n, header, re.M), n
        assert n in mg.EXPORTS and hasattr(L, n), n
    assert callable(mg.readset_clean_mods) and callable(mg.readset_properties)
