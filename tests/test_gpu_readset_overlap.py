"""modasm -o1 / -o2 / -b / -c on the device (mgReadsetFindOverlaps .. mgReadsetMarkContained: mg_overlap.hip) against the reference program's own
lines and files (tests/golden/ovl_*) and, on read sets built to sit on the kernels' edges, against the Python restatement that
tests/test_readset_overlap.py pins to the same reference output.  Everything is compared exactly: text, bytes, integers; every shape a test
is about is asserted (from the restatement or from mgReadsetOverlapsDiag), not assumed."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests import test_readset as trs
from tests import test_readset_overlap as tro
from tests import test_gpu_readset_clean as tgc
from tests import test_gpu_devsort as tds
from tests import overlap_designs as od

TAGS = tro.TAGS
W = 8
SORT_TILE = tds.MG_RSORT_TILE


# ---- the reference's fixture ----

@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_golden_sequences_on_the_device(tag, golden_dir, tmp_path):
    """every recorded command sequence, one fresh load each, path 0: the reference's lines, and ovl_<tag>_BC.* after -b -c"""
    tro.check_sequences_through_library(tag, golden_dir, tmp_path, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_host_loops_give_the_device_bytes(tag, golden_dir, tmp_path):
    L = mg.lib()
    seqs, _ = tro.sequences(tag)
    _, cmds, _ = seqs["bc"]
    got = {}
    for how in ("device", "host"):
        rs = L.mgReadsetLoad(tro.golden_stem(golden_dir, tag).encode())
        out = str(tmp_path / how)
        if how == "host":
            with tro.host_loops():
                text = tro.lib_run(rs, cmds, out + ".txt"); path = L.mgReadsetOverlapsPath()
        else:
            text = tro.lib_run(rs, cmds, out + ".txt"); path = L.mgReadsetOverlapsPath()
        assert path == (how == "host")
        lists = mg.readset_find_overlaps(rs, list(range(1, rs.contents.nReads + 1)), 0, None, want_lists=True) if how == "device" else None
        if how == "host":
            with tro.host_loops():
                lists = mg.readset_find_overlaps(rs, list(range(1, rs.contents.nReads + 1)), 0, None, want_lists=True)
        L.mgReadsetWrite(rs, out.encode())
        got[how] = (text, lists, gzip.open(out + ".mod").read(), trs.readset_mask(gzip.open(out + ".readset").read()), tro.lib_flags(rs))
        L.mgReadsetDestroy(rs)
    assert got["device"] == got["host"]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_overlap_example_runs_like_modasm(tag, golden_dir, tmp_path):
    """examples/overlap_file.c = `modasm -r ovl_<tag> -b -c -o2 1 -w out` on the library, from plain C: the first lines of the recorded "bc" sequence"""
    exe = str(tmp_path / "overlap_file")
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "overlap_file.c"),
                        "-o", exe, "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    stem = tro.golden_stem(golden_dir, tag)
    out = str(tmp_path / "out")
    r = subprocess.run([exe, stem, "1", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    want = tro.golden_out(tag, "bc").splitlines(True)
    n = len(tro.sequences(tag)[1])
    assert r.stdout == "".join(want[:3 + 1 + n]) and want[3 + n].startswith("RR") and want[4 + n].startswith("RH")
    assert "overlaps on the device" in r.stderr
    assert trs.readset_mask(gzip.open(out + ".readset").read()) == trs.readset_mask(gzip.open(stem + "_BC.readset").read())
    assert gzip.open(out + ".mod").read() == gzip.open(stem + "_BC.mod").read()


# ---- read sets on the kernels' edges, against the restatement ----

def mutate(s, rate, rng):
    s = s.copy()
    m = rng.random(len(s)) < rate
    s[m] = (s[m] + 1 + rng.integers(0, 3, int(m.sum()))) & 3
    return s


def edge_reads(seed):
    """about 60 reads of up to 400 hits over 9 kb of the genome, so that every read has many partners: plain ones on both strands, mutated,
    rearranged, with an inverted segment, duplicated; a read without hits, a tandem read (every mod a repeat), reads of more than 64 and of more
    than 256 hits"""
    rng = np.random.default_rng(seed)
    g = tgc.world(W)[0]
    cat = np.concatenate
    reads = [np.zeros(0, np.uint8), rng.integers(0, 2, 300).astype(np.uint8)]                       # no hits
    for i in range(40):
        a = int(rng.integers(2000, 10000)); n = int(rng.integers(300, 2600))
        s = g[a:a + n]
        if i % 3 == 1:
            s = tgc.rc(s)
        if i % 5 == 2:
            s = mutate(s, 0.02, rng)
        reads.append(s)
    for i in range(6):
        a = int(rng.integers(2000, 9000)); n = int(rng.integers(900, 2000)); c = int(rng.integers(200, n - 200))
        reads.append(cat([g[a + c:a + n], g[a:a + c]]))                                              # rearranged
        reads.append(cat([g[a:a + c], tgc.rc(g[a + c:a + n])]) if i % 2 else cat([g[a:a + c // 2], tgc.rc(g[a + c // 2:a + c]), g[a + c:a + n]]))
    reads.append(cat([g[5000:5600], g[5000:5600]]))                                                  # tandem: every mod a repeat
    reads.append(cat([g[7000:7300]] * 3))
    reads += [g[3000:6200], g[3000:6200], tgc.rc(g[3000:6200])]                                      # about 400 hits each, identical
    reads.append(g[2500:3400]); reads.append(g[3100:3500])                                           # contained in the long ones
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


_sets = {}


def edge_set(seed, tmp_path):
    """(rs, lib_arrays, info) of edge_reads (seed), ingested on the device; the arrays once per seed"""
    ms, rs = tgc.ingest(edge_reads(seed), W, tmp_path)
    if seed not in _sets:
        _sets[seed] = (trs.lib_arrays(rs), tro.ms_info(ms))
    return rs, _sets[seed][0], _sets[seed][1]


def run_both(rs, r, cmds, tmp_path):
    """the commands through the library (on the device) and through the restatement: same lines, same flags"""
    before = len(r.out)
    text = tro.lib_run(rs, cmds, str(tmp_path / "lines.txt"))
    assert mg.lib().mgReadsetOverlapsPath() == 0
    r.run(cmds)
    assert text == "".join(r.out[before:])
    assert tro.lib_flags(rs) == (r.bad, r.contained)
    return text


@pytest.mark.gpu
def test_edge_set_lists_and_shapes(tmp_path):
    """every read's list in one call: the records, the order inside ties; the pair kernel strides (a y of more than 64 and of more than 256
    hits), first and last match in different strides, a query without hits, one whose every mod repeats, identical reads"""
    rs, a, info = edge_set(1, tmp_path)
    n = len(a["nHit"])
    assert 55 <= n <= 70 and a["nHit"].max() <= 420
    r = tro.Restatement(a, info)
    want = [r.find_overlaps(x, 0) for x in range(1, n + 1)]
    got = mg.readset_find_overlaps(rs, list(range(1, n + 1)), 0, None, want_lists=True)
    assert mg.lib().mgReadsetOverlapsPath() == 0
    assert got == want and tro.lib_flags(rs)[0] == r.bad
    batches, cands, pairs, launches = mg.readset_overlaps_diag()
    assert (batches, cands, pairs, launches) == (1, sum(r.cands.values()), sum(len(l) for l in want), 1)
    assert cands > SORT_TILE                                                                  # more than one tile of the candidate sorts
    partners = {e[0] for l in want for e in l}
    assert any(a["nHit"][y - 1] > 256 for y in partners) and any(64 < a["nHit"][y - 1] <= 256 for y in partners)
    assert any(e[1] > 200 for l in want for e in l)                                          # matches spread over more than three strides of y
    assert any(a["nHit"][x - 1] == 0 for x in range(1, n + 1))
    tandem = [x for x in range(1, n + 1) if r.pure(x)[0] > 0 and 2 * r.pure(x)[0] == a["nCopy"][x - 1][1]]
    assert tandem and all(r.bad[x] & tro.BAD_REPEAT for x in tandem)
    flags = [e[4] for l in want for e in l]
    assert any(f & tro.F_CONTAINED for f in flags) and any(f == 0 for f in flags) and any(f & tro.F_SKIPPED for f in flags)
    assert any(e[2] for l in want for e in l) and any(e[3] for l in want for e in l)
    assert any(len({e[1] for e in l}) < len(l) for l in want)                                 # equal nHit inside one list
    mg.lib().mgReadsetDestroy(rs)


def subset_with_sum(values, target):
    """indices of a subset of `values` that sums to `target` (None if there is none)"""
    reach = {0: []}
    for i, v in enumerate(values):
        if v <= 0:
            continue
        for s, idx in list(reach.items()):
            if s + v <= target and s + v not in reach:
                reach[s + v] = idx + [i]
    return reach.get(target)


@pytest.mark.gpu
def test_candidates_exactly_one_sort_tile(tmp_path):
    """queries whose candidates are exactly MG_RSORT_TILE, and one more query: one tile, then two"""
    rs, a, info = edge_set(1, tmp_path)
    n = len(a["nHit"])
    r = tro.Restatement(a, info)
    for x in range(1, n + 1):
        r.pure(x)
    idx = subset_with_sum([r.cands[x] for x in range(1, n + 1)], SORT_TILE)
    assert idx, "no subset of the reads has exactly %d candidates" % SORT_TILE
    reads = [i + 1 for i in idx]
    extra = next(x for x in range(1, n + 1) if x not in reads and r.cands[x] > 0)
    for queries in (reads, reads + [extra]):
        want = [r.find_overlaps(x, 0) for x in queries]
        got = mg.readset_find_overlaps(rs, queries, 0, None, want_lists=True)
        assert got == want
        d = mg.readset_overlaps_diag()
        assert d[:2] == (1, sum(r.cands[x] for x in queries)) and mg.lib().mgReadsetOverlapsPath() == 0
    assert sum(r.cands[x] for x in reads) == SORT_TILE
    mg.lib().mgReadsetDestroy(rs)


@pytest.mark.gpu
def test_table_in_lds_and_in_hbm(tmp_path):
    """MODGPU_OVERLAP_LDS: tables that fit a wave's share of LDS and tables that do not, in one launch; all of them in HBM; the same lists"""
    rs, a, info = edge_set(2, tmp_path)
    n = len(a["nHit"])
    r = tro.Restatement(a, info)
    want = [r.find_overlaps(x, 0) for x in range(1, n + 1)]
    sizes = [r.table_size[x] for x in range(1, n + 1) if want[x - 1]]
    assert min(sizes) <= 64 < max(sizes)
    for cap in (64, 0, None):
        with mg.knobs(OVERLAP_LDS=cap):
            rs.contents.bad[0] = 0
            for i in range(1, n + 1):
                rs.contents.bad[i] = 0
            r2 = tro.Restatement(a, info)
            assert mg.readset_find_overlaps(rs, list(range(1, n + 1)), 0, None, want_lists=True) == [r2.find_overlaps(x, 0) for x in range(1, n + 1)]
            assert mg.lib().mgReadsetOverlapsPath() == 0
    mg.lib().mgReadsetDestroy(rs)


@pytest.mark.gpu
def test_batches_and_repeated_commands(tmp_path):
    """-b -c -b -c -o2 1 with one batch, with a budget that makes a few, and with one query per batch -- where every skip of another read is
    the work of an earlier batch: the same lines, flags and files; contained is never reset"""
    cmds = ["-b", "-c", "-o2", "3", "-b", "-c", "-c", "-o2", "1", "-o1", "7"]
    got = {}
    for budget in (None, 30000, 1):
        rs, a, info = edge_set(3, tmp_path)
        n = len(a["nHit"])
        r = tro.Restatement(a, info)
        with mg.knobs(OVERLAP_CANDS=budget):
            with mg.CFile(str(tmp_path / "b.txt"), "w") as f:
                assert mg.readset_mark_bad_reads(rs, f) == 0
            batches = mg.readset_overlaps_diag()[0]
            r.mark_bad_reads()
            assert open(tmp_path / "b.txt").read() == "".join(r.out) and tro.lib_flags(rs)[0] == r.bad
            empty = sum(1 for x in range(1, n + 1) if r.cands[x] == 0)                     # a query without candidates joins the batch before it
            assert batches == 1 if budget is None else 3 <= batches < n - empty if budget == 30000 else n - empty <= batches <= n
            text = run_both(rs, r, cmds, tmp_path)
        out = str(tmp_path / ("out%s" % budget))
        mg.lib().mgReadsetWrite(rs, out.encode())
        got[budget] = (text, gzip.open(out + ".mod").read(), trs.readset_mask(gzip.open(out + ".readset").read()))
        if budget == 1:
            r3 = tro.Restatement(a, info)
            seen = {x: r3.find_overlaps(x, 0) for x in range(1, n + 1)}
            assert any(e[4] & tro.F_SKIPPED and e[0] != x for x, l in seen.items() for e in l)
        assert any(r.contained) and any(r.bad) and not all(r.bad[1:])
        mg.lib().mgReadsetDestroy(rs)
    assert got[None] == got[30000] == got[1]


# ---- read sets built by design (tests/overlap_designs.py; the CPU leg is tests/test_readset_overlap.py) ----

def designed(name, tmp_path):
    """(rs, the restatement whose design properties are asserted) of a designed set ingested on the device: the arrays equal the oracle's (dx and
    len of set E among them); the designs, the oracle's arrays and the restatements once per process"""
    assert od.SORT_TILE == SORT_TILE
    _, rs = od.ingest(name, tmp_path)
    return rs, od.checked(name, *od.oracle_set(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "D", "E"])
def test_designed_sets_on_the_device(name, tmp_path):
    """A: partners of exactly 3 .. 193 hits, matches at lane 63 / lane 0, a stride without matches, a late first match, both strands, out-of-order
    matches whose previous match is the wave's carry, nPlus == nMinus, tandem reads, runs of 2 and 3, contained / overlap on both sides of
    equality.  B: a third of the hits not copy 1 (flag[] and place[] of the compaction are no identity; more than one scan tile), then candidate
    budgets of exactly the first batch's bounds and one less.  D: more pairs than one sort tile, 20 equal nHit across a tile line, nPairs of 1 and
    of every residue of 4, more than 1024 queries.  E: dx that wraps, positions past 2^16.  Every read's list in one call, then -o2 / -b / -c /
    -o1: lists, lines, flags and the diag totals (batches, candidates, pairs, launches) against the restatement, path 0"""
    rs, r0 = designed(name, tmp_path)
    od.run_set(name, rs, r0, tmp_path, 0)
    mg.lib().mgReadsetDestroy(rs)


@pytest.mark.gpu
def test_designed_tables_under_every_lds_setting(tmp_path):
    """C: tables of exactly 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049 and more than 2500 entries; MODGPU_OVERLAP_LDS = 64, unset, 2048 (the
    64 KiB launch), 4096 (clamped to 2048), 0 and -1: in each launch both paths (under 0 HBM alone), around each cap the pairs of the tables of cap
    and cap + 1 entries in one workgroup of four; identical results"""
    rs, r0 = designed("C", tmp_path)
    od.run_set("C", rs, r0, tmp_path, 0)
    mg.lib().mgReadsetDestroy(rs)
