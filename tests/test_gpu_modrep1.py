"""modrep -s1 / -s2 on the device (mgRepAnalyze1File, mgRepAnalyze1Hits, mgRepRunFinish1, mgRepAnalyze2File, mgRepCount2: mg_modrep1.hip)
against the reference program's own lines (tests/golden/rep1_*) and, on hit lists built to sit on the edges, against the restatement that
tests/test_modrep1.py pins to the same reference output.  Everything is compared exactly: text, integers, arrays."""
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests import test_modrep as tmr
from tests import test_modrep1 as tm1
from tests import test_gpu_devsort as tds

SORT_TILE, SCAN_TILE = tds.MG_RSORT_TILE, tds.MG_SCAN_TILE      # mg_devsort.h's (tests/test_abi.py holds them to the header)
K = 19
STALE_SEEDS = range(400)                                       # the seed budget of the search for a stale pre[0] read, on the CPU


def read_text(p):
    return open(p).read()


# ---- hit lists ----

def flat(lists):
    """per-read (k list, x list) -> (hitStart, hitK, hitX)"""
    hs = np.zeros(len(lists) + 1, np.uint64)
    hs[1:] = np.cumsum([len(k) for k, _ in lists])
    cat = lambda j: np.array([v for l in lists for v in l[j]], np.int32)
    return hs, cat(0), cat(1)


def check_hits(m, k, read_i, lists, tmp_path):
    """mgRepAnalyze1Hits equals the restatement: text, arrays, the diagnostics; returns (result, restatement's diag)"""
    w_out, w_err, w_res, w_diag = tm1.analyze1_end(m, k, read_i, lists)
    hs, hk, hx = flat(lists)
    res = mg.rep_analyze1_hits(m, k, read_i, hs, hk, hx, str(tmp_path / "o"), str(tmp_path / "e"))
    assert mg.lib().mgRepPath() == 0
    assert read_text(tmp_path / "o") == w_out and read_text(tmp_path / "e") == w_err
    w_res = dict(w_res, nRead=0, nBad=0, nGood=len(read_i))
    tmr.results_equal(res, w_res)
    d = mg.rep1_diag()
    assert {key: d[key] for key in w_diag} == w_diag and d["kernels"] > 0
    return res, w_diag


def walk_case(seed, n_reads, m, genome=120, length=(0, 80), drop=0.1):
    """reads as noisy stretches of one path of mods: genome[j] in 1 .. m - 1 (repeats when m is small), neighbours K - 1, K or K + 1 apart
    (now and then 3 K); a read is a stretch of it, each hit left out with probability `drop`; x counts from the stretch's first position"""
    rng = np.random.default_rng(seed)
    g = rng.integers(1, m, size=genome)
    pos = np.cumsum(rng.choice([K - 1, K, K + 1, 3 * K], size=genome, p=[0.25, 0.25, 0.25, 0.25]))
    lists = []
    for _ in range(n_reads):
        n = int(rng.integers(length[0], length[1] + 1))
        a = int(rng.integers(0, max(1, genome - n + 1)))
        keep = np.flatnonzero(rng.random(min(n, genome - a)) >= drop) + a
        lists.append((g[keep].tolist(), (pos[keep] - pos[a]).tolist() if len(keep) else []))
    return list(rng.permutation(1000)[:n_reads]), lists


_stale = {}


def stale_seed():
    """the first seed of STALE_SEEDS whose walk_case makes a verdict read a pre[0] that an earlier build left (found by the restatement)"""
    if "seed" not in _stale:
        _stale["seed"] = None
        for seed in STALE_SEEDS:
            read_i, lists = walk_case(seed, 24, 40, genome=60, length=(5, 40), drop=0.15)
            if tm1.analyze1_end(40, K, read_i, lists)[3]["stale"]:
                _stale["seed"] = seed
                break
    return _stale["seed"]


# ---- 1: the reference's fixture ----

def open_ref(golden_dir, err=None):
    ref_fa, ref_mod, _, _ = tm1.golden_paths(golden_dir)
    return mg.rep_ref_create(ref_fa, ref_mod, err)


@pytest.mark.gpu
def test_golden(golden_dir, tmp_path):
    """modrep -R rep_k19d8_ref.fa rep_k19d8_ref.mod -s1 rep1_reads.fa rep1_reads.mod -s2 rep1_reads.fa rep1_reads.mod: stdout, stderr,
    every array of the result, on the device: four builds, links, hits removed as runs"""
    L = mg.lib()
    w = tm1.world(golden_dir)
    _, _, reads_fa, reads_mod = tm1.golden_paths(golden_dir)
    ref = open_ref(golden_dir, str(tmp_path / "R.err"))
    res = mg.rep_analyze1_file(ref, reads_fa, reads_mod, str(tmp_path / "s1.out"), str(tmp_path / "s1.err"))
    assert L.mgRepPath() == 0
    d = mg.rep1_diag()
    assert d["builds"] == tm1.BUILDS and d["links"] > 0 and {key: d[key] for key in w["diag1"]} == w["diag1"]
    counts = mg.rep_analyze2_file(ref, reads_fa, reads_mod, str(tmp_path / "s2.out"))
    assert L.mgRepPath() == 0 and counts == w["counts2"]
    assert read_text(tmp_path / "s1.out") + read_text(tmp_path / "s2.out") == util.golden_text("rep1.stdout.txt")
    assert read_text(tmp_path / "R.err") + read_text(tmp_path / "s1.err") == util.golden_text("rep1.stderr.txt")
    tmr.results_equal(res, w["res1"])
    L.mgRepRefDestroy(ref)


@pytest.mark.gpu
def test_rep1_example_runs_like_modrep(golden_dir, tmp_path):
    """examples/rep1_file.c = `modrep -R ref.fa ref.mod -s1 reads.fa reads.mod -s2 reads.fa reads.mod` on the library, from plain C"""
    exe = str(tmp_path / "rep1_file")
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "rep1_file.c"),
                        "-o", exe, "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + list(tm1.golden_paths(golden_dir)), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    assert r.stdout == util.golden_text("rep1.stdout.txt")
    assert r.stderr == util.golden_text("rep1.stderr.txt")


# ---- 2: a file in batches; entry max ----

@pytest.mark.gpu
def test_batches(golden_dir, tmp_path):
    """the fixture's reads through one mgRepRunAdd and through three: the same lines and arrays"""
    L = mg.lib()
    w = tm1.world(golden_dir)
    _, _, _, reads_mod = tm1.golden_paths(golden_dir)
    ref = open_ref(golden_dir)
    p_ms, _ = tmr.load_set(reads_mod)
    reads = w["reads"]
    got = []
    for name, cuts in (("one", []), ("three", [7, 33])):
        parts = [reads[a:b] for a, b in zip([0] + cuts, cuts + [len(reads)])]
        res = mg.rep_run1(ref, p_ms, [util.concat_reads(list(b)) for b in parts], str(tmp_path / (name + ".out")), str(tmp_path / (name + ".err")))
        assert L.mgRepPath() == 0
        got.append((read_text(tmp_path / (name + ".out")), read_text(tmp_path / (name + ".err"))))
        tmr.results_equal(res, w["res1"])
    assert got[0] == got[1] == (w["out1"], w["err1"])
    tmr.destroy_set(p_ms)
    L.mgRepRefDestroy(ref)


@pytest.mark.gpu
def test_entry_max_is_refused(golden_dir, tmp_path):
    """a read that holds entry max of the second set: -1, the message, and nothing printed -- from the file, and from hit lists"""
    L = mg.lib()
    ref = open_ref(golden_dir)
    out, err = str(tmp_path / "o"), str(tmp_path / "e")
    with pytest.raises(mg.ModgpuError, match=tm1.REFUSAL):
        mg.rep_analyze1_file(ref, os.path.join(golden_dir, "rep1_max_reads.fa"), os.path.join(golden_dir, "rep1_max_reads.mod"), out, err)
    assert L.mgRepPath() == -1 and read_text(out) == "" and read_text(err) == ""
    read_i, lists = walk_case(3, 10, 8)
    lists[4] = (lists[4][0] + [8], lists[4][1] + [10 ** 6])
    with pytest.raises(mg.ModgpuError, match=tm1.REFUSAL):
        hs, hk, hx = flat(lists)
        mg.rep_analyze1_hits(8, K, read_i, hs, hk, hx, out, err)
    assert L.mgRepPath() == -1 and read_text(out) == "" and read_text(err) == ""
    L.mgRepRefDestroy(ref)


# ---- 3: hit lists on the edges ----

@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [10, 11, 24])
@pytest.mark.parametrize("m", [8, 300])
def test_random_hit_lists(n_reads, m, tmp_path):
    """thresh = reads / 2 for an even and an odd number of reads; a set of 8 entries under short reads (every class of the first cleanMods
    occurs: small, big, good) and one of 300 under long ones (runs, links, dropped reads)"""
    seen, classes = dict(runs=0, links=0, dropped=0), np.zeros(4, np.int64)
    for seed in range(6):
        read_i, lists = walk_case(100 * n_reads + seed, n_reads, m, genome=14 if m == 8 else 120, length=(0, 6) if m == 8 else (0, 80))
        res, diag = check_hits(m, K, read_i, lists, tmp_path)
        classes += res["nmod"][0]
        for key in seen:
            seen[key] += diag[key]
    assert classes.min() > 0 and (m == 8 or min(seen.values()) > 0), (classes, seen)


def prefix_reads(first, lengths, gaps):
    """reads that are the first `n` of the mods first, first + 1, .. for n in lengths; gaps[j]: the distance from hit j to hit j + 1"""
    pos = np.concatenate([[0], np.cumsum(gaps)])
    return [(list(range(first, first + n)), pos[:n].tolist()) for n in lengths]


@pytest.mark.gpu
def test_run_walk_wave_edges(tmp_path):
    """reads of 0, 1, 2, 63, 64, 65 and 200 hits whose every mod has a count inside [5, reads / 2], so they reach the run removal at that
    length; neighbours K - 1, K and K + 1 apart, so the chain of kept hits crosses the 64th hit in every phase"""
    rng = np.random.default_rng(7)
    gaps = rng.choice([K - 1, K, K + 1], size=200)
    lists = prefix_reads(1, [200] * 6 + [65, 64, 63, 2, 1, 0], gaps) + prefix_reads(201, [90] * 12, rng.choice([K - 1, K + 1], size=90))
    order = rng.permutation(24)
    lists = [lists[i] for i in order]
    res, diag = check_hits(300, K, list(range(24)), lists, tmp_path)
    assert res["nmod"][0].tolist() == [10, 0, 0, 290] and diag["runs"] > 500 and res["nmod"][1][0] > 10


@pytest.mark.gpu
def test_counts_on_the_thresholds(tmp_path):
    """24 reads, thresh 12, hits 2 K apart (no runs).  Mods in exactly 4 (a: small), 5 (b), 12 (c, and the first hits A and B) and 13 reads
    (d: big).  e follows B in 9 reads and nowhere else, so the first verdicts take it (no new info); then f follows B in exactly 4 reads
    (114 .. 117: a weak link, they are dropped) and g follows B in exactly 5 (118 .. 122: they stay)"""
    a, b, c, d, e, f, g, h, z, A, B = 1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 21
    lists = []
    for r in range(24):
        ks = [A if r < 12 else B]
        ks += [m for m, reads in ((a, 4), (b, 5), (c, 12), (d, 13)) if r < reads]
        if r < 5:
            ks += [f, z]
        if 14 <= r < 18:
            ks += [e, f, z]
        if 18 <= r < 23:
            ks += [e, g, h]
        lists.append((ks, [2 * K * j for j in range(len(ks))]))
    res, diag = check_hits(300, K, list(range(100, 124)), lists, tmp_path)
    assert res["nmod"][0].tolist() == [300 - 11, 1, 1, 9]
    assert diag["runs"] == 0 and diag["dropped"] == 4 and res["readsBefore"] == 24
    assert sorted(set(range(100, 124)) - set(res["readI"].tolist())) == [114, 115, 116, 117]


@pytest.mark.gpu
def test_more_links_than_a_sort_tile(tmp_path):
    """two families of 12 reads over 450 mods each, a tenth of the hits left out at random: about 9 700 links, more than a tile of the
    shared sort and more than two of the shared scan take"""
    rng = np.random.default_rng(11)
    lists = []
    for fam in range(2):
        gaps = rng.choice([2 * K, 3 * K], size=450)
        pos = np.concatenate([[0], np.cumsum(gaps)])
        for _ in range(12):
            keep = np.flatnonzero(rng.random(450) >= 0.1)
            lists.append(((1 + 450 * fam + keep).tolist(), pos[keep].tolist()))
    _, diag = check_hits(1000, K, list(range(24)), lists, tmp_path)
    assert diag["links"] > SORT_TILE and diag["links"] > 2 * SCAN_TILE and diag["entries"] > 1024


@pytest.mark.gpu
def test_stale_pre0_is_read_as_the_program_reads_it(tmp_path):
    """modrep.c:376 reads pre[0] of a mod whose pre list is empty: what the last non-empty build left there.  A seed whose hit lists make
    that happen with a non-zero entry is looked for on the CPU (STALE_SEEDS); the device then reports the same number of such reads"""
    seed = stale_seed()
    assert seed is not None, "no seed of the budget makes a verdict read a stale pre[0]"
    read_i, lists = walk_case(seed, 24, 40, genome=60, length=(5, 40), drop=0.15)
    _, diag = check_hits(40, K, read_i, lists, tmp_path)
    assert diag["stale"] > 0 and mg.rep1_diag()["stale"] == diag["stale"]


@pytest.mark.gpu
def test_empty_ends(tmp_path):
    """no read; reads without hits; one read"""
    check_hits(8, K, [], [], tmp_path)
    check_hits(8, K, [5, 6, 7], [([], []), ([], []), ([], [])], tmp_path)
    check_hits(8, K, [0], [([1, 2, 3], [0, 30, 60])], tmp_path)


# ---- 4: -s2 ----

@pytest.mark.gpu
def test_count2_order_and_empty_reads(golden_dir):
    """the counts do not depend on the reads' order or on the batches; an empty read and one shorter than k add nothing"""
    L = mg.lib()
    w = tm1.world(golden_dir)
    ref = open_ref(golden_dir)
    reads = list(w["reads"])
    want = w["counts2"]
    assert mg.rep_count2(ref, *util.concat_reads(reads)) == want and L.mgRepPath() == 0
    swapped = list(reads)
    s2 = [i for i, n in enumerate(w["names"]) if n.startswith("s2_")]
    swapped[s2[0]], swapped[s2[-1]] = swapped[s2[-1]], swapped[s2[0]]
    assert mg.rep_count2(ref, *util.concat_reads(swapped)) == want
    more = reads[:5] + [reads[0][:0], reads[0][:K - 1]] + reads[5:]
    assert mg.rep_count2(ref, *util.concat_reads(more)) == want
    c = mg.rep_count2(ref, *util.concat_reads(reads[:20]))
    assert mg.rep_count2(ref, *util.concat_reads(reads[20:]), counts=c) == want
    assert mg.rep_count2(ref, *util.concat_reads([reads[0][:0], reads[0][:K - 1]])) == [0, 0, 0, 0]
    L.mgRepRefDestroy(ref)
