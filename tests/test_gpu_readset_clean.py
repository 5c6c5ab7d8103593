"""modasm -C and -P on the device (mgReadsetCleanMods, mgReadsetProperties: mg_rsdev.hip) against the reference program's own files and
lines (tests/golden/clean_*) and, on reads built to sit on the edges, against the numpy restatement that tests/test_readset_clean.py pins
to the same reference output.  Everything is compared exactly: bytes, integers, text."""
import contextlib
import gzip
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests import test_readset as trs
from tests import test_readset_clean as trc
from tests.test_readset_clean import MS_MINOR, MS_REPEAT, MS_INTERNAL, MS_RDNA, TOPMASK
from tests import test_gpu_devsort as tds

TAGS = trc.TAGS
K = 15
SORT_TILE = tds.MG_RSORT_TILE   # mg_devsort.h's (tests/test_abi.py holds it to the header): elements per workgroup of a sort pass


def read_text(p):
    return open(p).read()


def info_of(rs):
    return trc.ms_arrays(rs.contents.ms)[1]


# ---- 1, 2, 3, 5, 6: the reference's fixture ----

@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_golden_clean_mods(tag, golden_dir, tmp_path):
    """modasm -r clean_<tag> -C -w out: the line, the .mod bytes, the .readset but for its addresses; on the device; a second -C changes nothing"""
    L = mg.lib()
    stem = trc.golden_stem(golden_dir, tag)
    rs = L.mgReadsetLoad(stem.encode())
    for again in range(2):
        assert mg.readset_clean_mods(rs, str(tmp_path / "c.txt")) == 0
        assert read_text(tmp_path / "c.txt") == trc.golden_lines(tag)[0]
        out = str(tmp_path / ("out%d" % again))
        L.mgReadsetWrite(rs, out.encode())
        trc.written_equals_golden(out, stem + "_C")
    L.mgReadsetDestroy(rs)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_golden_properties(tag, golden_dir, tmp_path):
    """modasm -r clean_<tag> -P: the reference's MT / READ / RM lines; on the device; the set is left as it was"""
    L = mg.lib()
    rs = L.mgReadsetLoad(trc.golden_stem(golden_dir, tag).encode())
    before, info0 = trs.lib_arrays(rs), info_of(rs)
    assert mg.readset_properties(rs, str(tmp_path / "p.txt")) == 0
    text = read_text(tmp_path / "p.txt")
    assert text == trc.golden_lines(tag)[1]
    assert "MT i " in text and "\nRM " in text
    assert np.array_equal(info_of(rs), info0)
    trs.same(before, trs.lib_arrays(rs))
    L.mgReadsetDestroy(rs)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_ingest_then_clean_in_one_process(tag, golden_dir, tmp_path):
    """modasm -m clean_<tag>_src.mod -f clean_<tag>_reads.fa -C -P -w out: the hit lists made by this process, the device table of the
    set alive when -C changes info[]"""
    L = mg.lib()
    stem = trc.golden_stem(golden_dir, tag)
    ms = trs.load_mod_gz(stem + "_src.mod", str(tmp_path / "src.mod"))
    rs = L.mgReadsetCreate(ms)
    assert L.mgReadsetFileRead(rs, (stem + "_reads.fa").encode()) == 0
    assert mg.readset_clean_mods(rs, str(tmp_path / "c.txt")) == 0
    assert mg.readset_properties(rs, str(tmp_path / "p.txt")) == 0
    assert (read_text(tmp_path / "c.txt"), read_text(tmp_path / "p.txt")) == trc.golden_lines(tag)
    out = str(tmp_path / "out")
    L.mgReadsetWrite(rs, out.encode())
    trc.written_equals_golden(out, stem + "_C", mod_mask=trs.mod_mask)
    L.mgReadsetDestroy(rs)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_host_loops_give_the_device_bytes(tag, golden_dir, tmp_path):
    """the same set through the device and through the host loops (MODGPU_READSET_HOST=1 + mgReloadKnobs): the same lines and files"""
    L = mg.lib()
    stem = trc.golden_stem(golden_dir, tag)
    got = {}
    for how in ("device", "host"):
        rs = L.mgReadsetLoad(stem.encode())
        c, p, out = (str(tmp_path / (how + e)) for e in (".c.txt", ".p.txt", ""))
        if how == "host":
            with trc.host_loops():
                assert (mg.readset_clean_mods(rs, c), mg.readset_properties(rs, p)) == (1, 1)
        else:
            assert (mg.readset_clean_mods(rs, c), mg.readset_properties(rs, p)) == (0, 0)
        L.mgReadsetWrite(rs, out.encode())
        got[how] = (read_text(c), read_text(p), gzip.open(out + ".mod").read(), trs.readset_mask(gzip.open(out + ".readset").read()), trs.lib_arrays(rs))
        L.mgReadsetDestroy(rs)
    assert got["device"][:4] == got["host"][:4]
    trs.same(got["device"][4], got["host"][4])


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_device_table_follows_the_new_info(tag, golden_dir, tmp_path):
    """-C on a set whose table is on the device: mgModsetWriteTextDevice afterwards shows the new info column, as mgModsetWriteText does from
    the host arrays"""
    L = mg.lib()
    stem = trc.golden_stem(golden_dir, tag)
    ms = trs.load_mod_gz(stem + "_src.mod", str(tmp_path / "src.mod"))
    rs = L.mgReadsetCreate(ms)
    assert L.mgReadsetFileRead(rs, (stem + "_reads.fa").encode()) == 0
    mg.write_text_device(ms, str(tmp_path / "before.txt"))                       # the device table exists, with the info of before
    assert mg.readset_clean_mods(rs, str(tmp_path / "c.txt")) == 0
    mg.write_text_device(ms, str(tmp_path / "device.txt"))
    with mg.CFile(str(tmp_path / "host.txt"), "w") as f:
        L.mgModsetWriteText(ms, f)
    assert read_text(tmp_path / "device.txt") == read_text(tmp_path / "host.txt") != read_text(tmp_path / "before.txt")
    L.mgReadsetDestroy(rs)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_clean_example_runs_like_modasm(tag, golden_dir, tmp_path):
    """examples/clean_file.c = `modasm -r clean_<tag> -C -P -w out` on the library, from plain C"""
    exe = str(tmp_path / "clean_file")
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "clean_file.c"),
                        "-o", exe, "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    stem = trc.golden_stem(golden_dir, tag)
    out = str(tmp_path / "out")
    r = subprocess.run([exe, stem, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    assert r.stdout == util.golden_text("clean_%s.stdout.txt" % tag)
    assert "-C on the device, -P on the device" in r.stderr
    trc.written_equals_golden(out, stem + "_C")


# ---- 4: reads on the edges, against the restatement ----

_worlds = {}


def world(w):
    """(genome, the sorted positions of its seeds, the .mod bytes of the oracle's set of its k-mers and of poly-A, copy classes by -s 1 2 3): once per w"""
    if w not in _worlds:
        from oracle import pyoracle as orc
        import tempfile
        g = util.without_two_letter_windows(np.random.default_rng(4100 + w).integers(0, 4, 40_000).astype(np.uint8), K)
        h = orc.Hasher(K, w, 17); oms = orc.Modset(h, 20)
        oms.add_sequence(np.zeros(100, np.uint8)); oms.add_sequence(g)
        oms.set_copy(1, 2, 3)
        with tempfile.TemporaryDirectory() as d:
            oms.write_mod(os.path.join(d, "m.mod"))
            _worlds[w] = (g, np.sort(h.scan(g)[1].astype(np.int64)), open(os.path.join(d, "m.mod"), "rb").read())
        _worlds[w, "seeds"] = (h, np.unique(np.concatenate([h.scan(g)[0], h.scan(np.zeros(K, np.uint8))[0]])))
        oms.close()
    return _worlds[w]


def hits_of(w, read):
    """the hits a read is going to have: its seeds that are k-mers of the set (a read glued from pieces of the genome can hold a k-mer of the
    genome across a joint)"""
    world(w)
    h, seeds = _worlds[w, "seeds"]
    return int(np.isin(h.scan(read)[0], seeds).sum())


def rc(s):
    return (3 - s[::-1]).astype(np.uint8)


class Reads:
    """reads made of pieces of the genome, with the number of the hit each is going to begin at"""
    def __init__(self, w, seed):
        self.w = w
        self.g, self.pos, _ = world(w)
        self.rng = np.random.default_rng(seed)
        self.reads, self.start, self.tot, self.at = [], [], 0, {}

    def hits(self, a, b):
        return int(np.searchsorted(self.pos, b - K, "right") - np.searchsorted(self.pos, a, "left")) if b - a >= K else 0

    def add(self, r, name=None):
        if name:
            self.at[name] = len(self.reads)
        self.reads.append(np.ascontiguousarray(r, np.uint8)); self.start.append(self.tot); self.tot += hits_of(self.w, self.reads[-1])

    def cut(self, a, b, name=None, flip=False):
        self.add(rc(self.g[a:b]) if flip else self.g[a:b], name)

    def end_with(self, a, n):
        """b with exactly n seeds in g[a:b]"""
        b = a + K
        while self.hits(a, b) < n:
            b += 1
        return b

    def tandem(self, a, n, name):
        """g[a:b] twice, n seeds each"""
        b = self.end_with(a, n)
        self.add(np.concatenate([self.g[a:b], self.g[a:b]]), name)

    def fill_to(self, target):
        """plain reads, both strands, until exactly `target` hits stand before the next read"""
        assert self.tot <= target
        while target - self.tot > 700:
            a = int(self.rng.integers(0, 33_000)); self.cut(a, a + int(self.rng.integers(800, 1500)), flip=bool(self.rng.integers(0, 2)))
        if target > self.tot:
            a = int(self.rng.integers(0, 30_000)); self.cut(a, self.end_with(a, target - self.tot))
        assert self.tot == target


def edge_reads(w, seed, target):
    """reads with 0 .. 3 hits and more, a read that holds its mods forward and reverse, one that holds them three times, a tandem read whose
    two halves lie on either side of hit number `target` (an edge of the sort's tiles), and last a tandem read of mods no other read repeats"""
    R = Reads(w, seed)
    R.add(np.zeros(0, np.uint8)); R.cut(100, 110); R.add(R.rng.integers(0, 2, 300), "junk")
    for _ in range(60):
        a = int(R.rng.integers(20_000, 30_000)); R.cut(a, a + K + int(R.rng.integers(0, 4 * w)), flip=bool(R.rng.integers(0, 2)))
    b = R.end_with(6000, 150)
    R.add(np.concatenate([R.g[6000:b], rc(R.g[6000:b])]), "fwd_rev")
    b = R.end_with(7000, 40)
    R.add(np.concatenate([R.g[7000:b]] * 3), "thrice")
    R.cut(6800, 7060, "across")                                                  # from mods that it alone hits into the ones hit three times more: minor variants
    if target:
        R.fill_to(target - 100)
    R.tandem(1000, 200, "tandem_mid")
    for _ in range(3):
        a = int(R.rng.integers(0, 33_000)); R.cut(a, a + 1200)
    R.tandem(36_000, 50, "tandem_last")
    return R


def ingest(reads, w, tmp_path):
    L = mg.lib()
    p = str(tmp_path / "m.mod"); open(p, "wb").write(world(w)[2])
    with mg.CFile(p, "r") as f:
        ms = L.modsetRead(f)
    rs = L.mgReadsetCreate(ms)
    bases, offs = util.concat_reads(reads)
    assert L.mgReadsetRead(rs, bases.ctypes.data, offs.ctypes.data, len(reads)) == 0
    return ms, rs


def preload_info(ms, seed):
    """copy classes flipped, MS_RDNA, MS_MINOR and the flags of an earlier -C on some mods: written into the host array, the library told"""
    rng = np.random.default_rng(seed)
    info = np.ctypeslib.as_array(ms.contents.info, (ms.contents.max + 1,))
    n = len(info) - 1
    x = rng.random(n)
    new = info[1:].copy()
    flip = x < 0.3
    new[flip] = (new[flip] & 0xfc) | rng.integers(0, 4, int(flip.sum())).astype(np.uint8)
    new[rng.random(n) < 0.1] |= MS_RDNA
    new[rng.random(n) < 0.05] |= MS_MINOR
    new[rng.random(n) < 0.02] |= MS_REPEAT | MS_INTERNAL
    new[rng.random(n) < 0.01] |= 0xc0                                            # the two bits modset.h leaves unnamed
    info[1:] = new
    mg.lib().mgModsetHostChanged(ms)


def check_against_restatement(ms, rs, w, tmp_path, want_path=0):
    """-P, -C, -C again, -P on the set as it stands, every result against the restatement on the test's own copies; returns (hit lists, info
    before, info after)"""
    a = trs.lib_arrays(rs)
    depth, info = (x.copy() for x in trc.ms_arrays(ms))
    want_info, want_line, want_nc = trc.clean_mods(a, depth, info, w)
    want_p = trc.read_properties(a, info)
    c, p = str(tmp_path / "c.txt"), str(tmp_path / "p.txt")
    assert mg.readset_properties(rs, p) == want_path
    assert read_text(p) == want_p
    assert np.array_equal(info_of(rs), info)
    trs.same(a, trs.lib_arrays(rs))
    for again in range(2):
        assert mg.readset_clean_mods(rs, c) == want_path
        assert read_text(c) == want_line
        got_depth, got_info = trc.ms_arrays(ms)
        assert np.array_equal(got_info, want_info) and np.array_equal(got_depth, depth)
        b = trs.lib_arrays(rs)
        assert np.array_equal(b["nCopy"], want_nc)
        trs.same({k: v for k, v in a.items() if k != "nCopy"}, {k: v for k, v in b.items() if k != "nCopy"})
    assert mg.readset_properties(rs, p) == want_path
    assert read_text(p) == want_p
    return a, info, want_info


def occurrences_straddle(a, r, edge, select=None):
    """does some mod of read r (row r of the arrays) occur in it on either side of element number `edge`, among the hits that `select` keeps?"""
    s, e = int(a["hitStart"][r]), int(a["hitStart"][r + 1])
    keep = np.ones(len(a["hit"]), bool) if select is None else select
    place = np.cumsum(keep) - 1                                                   # a kept hit's number among the kept ones
    m = a["hit"][s:e] & TOPMASK
    for x in np.unique(m):
        at = place[s:e][(m == x) & keep[s:e]]
        if len(at) >= 2 and at[0] < edge <= at[-1]:
            return True
    return False


def copy1_hits(a, info):
    return (info[a["hit"] & TOPMASK] & 3) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("target,host", [(0, False), (SORT_TILE, False), (2 * SORT_TILE, False), (SORT_TILE, True)])
def test_edges_vs_restatement(target, host, tmp_path):
    """w = 3.  Reads with 0, 1, 2, 3 hits (the internal rule needs three); a mod forward and reverse in one read; one three times; a repeat only
    in the last read; info pre-loaded with MS_RDNA, MS_MINOR, flags of an earlier -C and mixed copy classes between the ingest and the call
    (mgModsetHostChanged), which all survive and show in nCopy; and, for the two targets, just over 8192 and 2 * 8192 hits with a tandem
    read's two halves on either side of the edge -- in the hits that -C sorts and, before the classes are mixed, in the copy-1 hits that -P
    sorts.  host: the same through the host loops."""
    w = 3
    L = mg.lib()
    R = edge_reads(w, 77 + target, target)
    ms, rs = ingest(R.reads, w, tmp_path)
    a0 = trs.lib_arrays(rs)
    assert np.array_equal(a0["hitStart"][:-1], np.array(R.start)) and a0["totHit"] == R.tot      # the reads hold the hits they were cut for
    assert {0, 1, 2, 3} <= set(a0["nHit"].tolist())
    if target:
        info0 = info_of(rs)
        assert target < a0["totHit"] < target + 6000
        assert occurrences_straddle(a0, R.at["tandem_mid"], target) and occurrences_straddle(a0, R.at["tandem_mid"], target, select=copy1_hits(a0, info0))
        with trc.host_loops() if host else contextlib.nullcontext():
            assert mg.readset_properties(rs, str(tmp_path / "p0.txt")) == int(host)
        assert read_text(tmp_path / "p0.txt") == trc.read_properties(a0, info0)
    preload_info(ms, 5 + target)
    with trc.host_loops() if host else contextlib.nullcontext():
        a, info, info2 = check_against_restatement(ms, rs, w, tmp_path, want_path=int(host))
    assert not np.array_equal(trs.lib_arrays(rs)["nCopy"], a0["nCopy"])          # the copy classes were flipped: nCopy is rebuilt from them
    flags = np.uint8(MS_REPEAT | MS_INTERNAL | MS_MINOR)
    assert ((info2 & ~flags) == (info & ~flags)).all() and ((info2 & info) == info).all()      # every bit that was set stays; only the three flags are new
    new = info2 & ~info
    assert (new & MS_REPEAT).any() and (new & MS_INTERNAL).any() and (new & MS_MINOR).any()
    mods = lambda name: np.unique(a["hit"][int(a["hitStart"][R.at[name]]):int(a["hitStart"][R.at[name] + 1])] & TOPMASK)
    assert R.at["tandem_last"] == len(R.reads) - 1 and not (new[mods("tandem_last")] & MS_REPEAT).any()
    assert (info2[mods("tandem_mid")] & MS_REPEAT).all() and (info2[mods("fwd_rev")] & MS_REPEAT).all()      # orientation ignored
    text = read_text(tmp_path / "p.txt")
    for name, what in (("fwd_rev", "n2Rev"), ("tandem_mid", "n2Tan"), ("tandem_last", "n2Tan"), ("thrice", "nMoreTan")):
        line = [l for l in text.splitlines() if l.startswith("READ %d " % (R.at[name] + 1))][0].split()
        assert int(line[line.index(what) + 1]) > 5, (name, line)
    assert "MT i %d h " % (R.at["thrice"] + 1) in text and "RM %d nMoreTan " % (R.at["thrice"] + 1) in text
    L.mgReadsetDestroy(rs); L.modsetDestroy(ms)


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [1, 2])
def test_one_and_two_reads(n_reads, tmp_path):
    """the last read contributes nothing to -C: one tandem read alone sets no flag at all, of two only the first counts; -P prints both"""
    w = 3
    L = mg.lib()
    R = Reads(w, 3)
    R.tandem(1000, 60, "first")
    if n_reads == 2:
        R.tandem(36_000, 50, "last")
    ms, rs = ingest(R.reads, w, tmp_path)
    a, info, info2 = check_against_restatement(ms, rs, w, tmp_path)
    first = np.unique(a["hit"][:int(a["hitStart"][1])] & TOPMASK)
    if n_reads == 1:
        assert np.array_equal(info, info2) and read_text(tmp_path / "c.txt") == "set 0 repeated, 0 internal, 0 minor_variant mods\n"
    else:
        assert np.array_equal(np.flatnonzero(info2 & MS_REPEAT), first) and read_text(tmp_path / "c.txt").startswith("set 60 repeated, ")
    assert [l.split()[:6] for l in read_text(tmp_path / "p.txt").splitlines()] == [["READ", str(i + 1), "n", str(n), "n2Tan", str(n)] for i, n in enumerate([60, 50][:n_reads])]
    L.mgReadsetDestroy(rs); L.modsetDestroy(ms)


@pytest.mark.gpu
def test_saturated_mod_vs_restatement(tmp_path):
    """w = 1, poly-A hit more than 65 535 times: its depth is 65 535, so the 2 x comparisons of the minor rule run at the top of the range
    against its neighbours in a read; a repeat in a read that also holds it; the saturated mod counts as a repeat itself (no key past the
    last mod in this sort); made copy 1 on the host, it is one run of 69 986 hits in -P"""
    w = 1
    L = mg.lib()
    g, _, _ = world(w)
    poly = lambda n: np.zeros(n, np.uint8)
    reads = [g[3000:4000], poly(70_000), np.concatenate([g[5000:5600], poly(40), g[7000:7600]]),
             np.concatenate([g[1000:1400], poly(30), g[1000:1400]]), rc(g[5200:7400]), g[900:1500], np.concatenate([g[36_000:36_200]] * 2)]
    ms, rs = ingest(reads, w, tmp_path)
    depth = trc.ms_arrays(ms)[0]
    sat = int(np.argmax(depth))
    assert depth[sat] == 65535 and (depth == 65535).sum() == 1
    preload_info(ms, 9)
    np.ctypeslib.as_array(ms.contents.info, (ms.contents.max + 1,))[sat] = 1      # copy 1, no flag
    L.mgModsetHostChanged(ms)
    a, info, info2 = check_against_restatement(ms, rs, w, tmp_path)
    assert info2[sat] & MS_REPEAT and not ((info2 & ~info) & MS_INTERNAL).any()  # w = 1: no distance is below it
    m = a["hit"] & TOPMASK
    s, e = int(a["hitStart"][2]), int(a["hitStart"][3])
    at = s + np.flatnonzero(m[s:e] == sat)
    assert len(at) >= 40 - K + 1 and s < at[0] and at[-1] + 1 < e and (info2[m[at[0] - 1]] & MS_MINOR) and (info2[m[at[-1] + 1]] & MS_MINOR) and 2 * int(depth[m[at[0] - 1]]) < 65535
    u, c = np.unique(m[int(a["hitStart"][3]):int(a["hitStart"][4])], return_counts=True)
    assert sat in u[c >= 2] and (c >= 2).sum() > 300 and (info2[u[c >= 2]] & MS_REPEAT).all()
    assert "MT i 2 h %d count %d\n" % (sat, 70_000 - K + 1) in read_text(tmp_path / "p.txt")
    L.mgReadsetDestroy(rs); L.modsetDestroy(ms)


# ---- 7: more seeds than the first guess provides for ----

@pytest.mark.gpu
def test_ingest_retries_when_the_seed_guess_is_too_small(tmp_path):
    """mgReadsetSeedsDevice sizes its three seed arrays for min (bases / w * 1.5 + 65536, bases + 1) seeds; a batch with more has them freed and
    made again at the size the scan asked for, in the middle of the call.  w = 2 and four reads of 100 000 a, whose one k-mer is a modimizer
    at every start: 4 x 99 986 seeds against a guess of 367 118.  Ordinary reads, one that hits nothing, an empty one and one shorter than k
    stand between them.
    The hit lists, distances, counts and depths against the oracle's read set, exactly."""
    from oracle import pyoracle as orc
    w = 2
    h = orc.Hasher(K, w, 17)
    assert len(h.scan(np.zeros(K, np.uint8))[0]) == 1                             # the k-mer of a run of a IS a modimizer: the run is all seeds
    g = np.random.default_rng(4200).integers(0, 4, 20_000).astype(np.uint8)
    poly = np.zeros(100_000, np.uint8)
    reads = [poly, g[3000:3400], poly, rc(g[5000:5600]), poly, np.zeros(0, np.uint8), g[100:110], poly, g[900:1500], np.random.default_rng(4201).integers(0, 4, 500).astype(np.uint8)]
    total = sum(len(r) for r in reads)
    guess = total // w
    guess = min(guess + guess // 2 + 65536, total + 1)                            # mg_chain.hip, mgReadsetSeedsDevice
    oms = orc.Modset(h, 20)
    oms.add_sequence(np.zeros(100, np.uint8)); oms.add_sequence(g)
    oms.set_copy(1, 2, 3)
    ors = orc.Readset(oms); ors.read(reads)
    want = ors.arrays()
    p = str(tmp_path / "m.mod"); oms.write_mod(p)
    L = mg.lib()
    with mg.CFile(p, "r") as f:
        ms = L.modsetRead(f)
    rs = L.mgReadsetCreate(ms)
    bases, offs = util.concat_reads(reads)
    assert L.mgReadsetRead(rs, bases.ctypes.data, offs.ctypes.data, len(reads)) == 0
    got = trs.lib_arrays(rs)
    seeds = int(got["nHit"].sum() + got["nMiss"].sum())
    print("first guess %d, seeds of the batch %d" % (guess, seeds))
    assert guess < seeds <= total                                                 # the first attempt was too small: the call went round again
    trs.same(want, got)
    assert np.array_equal(trc.ms_arrays(ms)[0], oms.depths())
    assert int(oms.depths().max()) == 65535 and len(set(got["nHit"].tolist())) >= 5 and got["nMiss"].any()
    L.mgReadsetDestroy(rs); L.modsetDestroy(ms)
    ors.close(); oms.close()
