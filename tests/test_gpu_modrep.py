"""modrep -R / -s3 on the device (mgRepRefCreate, mgRepAnalyze3File, mgRepRunAdd: mg_modrep.hip) against the reference program's own
lines (tests/golden/rep_*) and, on reads built to sit on the edges, against the numpy restatement that tests/test_modrep.py pins to the
same reference output.  Everything is compared exactly: text, integers, arrays."""
import json
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import synth
from tests import util
from tests import test_modrep as tmr
from tests import test_gpu_devsort as tds

TAGS = tmr.TAGS
SORT_TILE = tds.MG_RSORT_TILE   # mg_devsort.h's (tests/test_abi.py holds it to the header): elements per workgroup of a sort pass
K, W = 15, 2                    # the edge tests: a few thousand bases give thousands of hits


def read_text(p):
    return open(p).read()


def run(ref, ms, batches, tmp_path, name="r"):
    """(stdout text, stderr text, result) of mgRepRunBegin / Add ... / Finish; the run went through the device kernels"""
    out, err = str(tmp_path / (name + ".out")), str(tmp_path / (name + ".err"))
    res = mg.rep_run(ref, ms, [util.concat_reads(list(b)) for b in batches], out, err)
    assert mg.lib().mgRepPath() == 0
    return read_text(out), read_text(err), res


# ---- 1: the reference's fixture ----

@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_golden(tag, golden_dir, tmp_path):
    """modrep -R rep_<tag>_ref.fa rep_<tag>_ref.mod -s3 rep_<tag>_reads.fa rep_<tag>_reads.mod: stdout, stderr, on the device, every array"""
    L = mg.lib()
    w = tmr.world(golden_dir, tag)
    ref_fa, ref_mod, reads_fa, reads_mod = tmr.golden_paths(golden_dir, tag)
    ref = mg.rep_ref_create(ref_fa, ref_mod, str(tmp_path / "R.err"))
    r = ref.contents
    m = r.ms.contents.max
    assert m == w["rs"].max and r.len == w["ref"]["len"]
    assert np.array_equal(np.ctypeslib.as_array(r.pos, (m + 1,)), w["ref"]["pos"]) and np.array_equal(np.ctypeslib.as_array(r.isF, (m + 1,)).astype(np.uint8), w["ref"]["isF"])
    res = mg.rep_analyze3_file(ref, reads_fa, reads_mod, str(tmp_path / "s3.out"), str(tmp_path / "s3.err"))
    assert L.mgRepPath() == 0
    assert read_text(tmp_path / "s3.out") == util.golden_text("rep_%s.stdout.txt" % tag)
    assert read_text(tmp_path / "R.err") + read_text(tmp_path / "s3.err") == util.golden_text("rep_%s.stderr.txt" % tag)
    tmr.results_equal(res, w["res"])
    L.mgRepRefDestroy(ref)


# ---- 2: the hits lie in the ORIENTED read ----

@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_oriented_hits(tag, golden_dir, tmp_path):
    """(k, x) of every good read = the library's host iterator on the read, reverse-complemented in numpy if it was flipped, looked up in
    the second set with a dict: even k included"""
    L = mg.lib()
    w = tmr.world(golden_dir, tag)
    ref_fa, ref_mod, reads_fa, reads_mod = tmr.golden_paths(golden_dir, tag)
    ref = mg.rep_ref_create(ref_fa, ref_mod)
    res = mg.rep_analyze3_file(ref, reads_fa, reads_mod, str(tmp_path / "o"), str(tmp_path / "e"))
    p_ms, _ = tmr.load_set(reads_mod)
    value, _, _ = mg.modset_arrays(p_ms)
    index = {int(v): i for i, v in enumerate(value) if i}
    sh = ref.contents.ms.contents.hasher
    flipped = 0
    for g, i in enumerate(res["goodI"]):
        s = w["reads"][i]
        if not res["isF"][i]:
            s = tmr.rc(s); flipped += 1
        kmer, pos, _ = mg.iterate(sh, s)
        want = [(index[int(u)], int(p)) for u, p in zip(kmer, pos) if int(u) in index]
        a, b = res["hitStart"][g], res["hitStart"][g + 1]
        assert list(zip(res["hitK"][a:b].tolist(), res["hitX"][a:b].tolist())) == want, (g, i)
    assert 0 < flipped < res["nGood"]
    tmr.destroy_set(p_ms)
    L.mgRepRefDestroy(ref)


# ---- a genome whose modimizers are all different, its set, its reference: once ----

_edge = {}


def edge_world():
    """dict(g; loc, isf: the genome's modimizers in order, modimizer j being entry j + 1 of the set; ms: Modset* of the genome; rs: its RepSet;
    ref: MgRepRef* of the genome against it; rref: the restatement's)"""
    if not _edge:
        L = mg.lib()
        h = tmr.pyoracle.Hasher(K, W, 17)
        for seed in range(7100, 7140):
            g = synth.iid_bases(2 * (2 * SORT_TILE + 3) + 1600, seed)
            kmer, loc, isf = h.scan(g)
            if len(np.unique(kmer)) == len(kmer) and len(kmer) >= 2 * SORT_TILE + 3 + 300:
                break
        else:
            raise AssertionError("no genome without a repeated modimizer")
        ms = mg.modsetCreate(mg.seqhashCreate(K, W, 17), 20)
        bases, offs = util.concat_reads([g])
        assert mg.add_sequence_batch(ms, bases, offs) == len(kmer)
        mg.check(L.modsetSyncToHost(ms, 0))
        rs = tmr.set_of(ms)
        assert rs.max == len(kmer) and np.array_equal(rs.find(kmer), np.arange(1, len(kmer) + 1))
        ref = mg.rep_ref_from_arrays(ms, g)
        _edge.update(g=g, loc=loc, isf=isf, ms=ms, rs=rs, ref=ref, rref=tmr.ref_create(rs, g))
    return _edge


def piece(e, first, count):
    """the stretch of the genome that holds exactly its modimizers first .. first + count - 1 (from 0), and no other"""
    return e["g"][int(e["loc"][first]):int(e["loc"][first + count - 1]) + K]


def check_run(e, batches, tmp_path, ms=None, rms=None):
    """the run equals the restatement's, text and arrays; returns the result"""
    ms, rms = ms or e["ms"], rms or e["rs"]
    out, err, res = run(e["ref"], ms, batches, tmp_path)
    w_out, w_err, w_res = tmr.analyze3(e["rs"], e["rref"], rms, [s for b in batches for s in b])
    assert out == w_out and err == w_err
    tmr.results_equal(res, w_res)
    return res


# ---- 3: the vote ----

@pytest.mark.gpu
def test_vote_edges(tmp_path):
    """reads cut from the reference between its own modimizers, so the counts are known: 99 / 100 / 101 hits; the (seqF, seqR) on both sides
    of `> 10`; a strand switch after the 100th hit"""
    e = edge_world()
    fr = lambda f, r: np.concatenate([piece(e, 500, f), tmr.rc(piece(e, 900, r))])
    reads = [piece(e, 10, 99), piece(e, 10, 100), piece(e, 10, 101), tmr.rc(piece(e, 10, 99)), tmr.rc(piece(e, 10, 100)),
             fr(10, 90), fr(11, 89), fr(11, 11), fr(50, 50), fr(90, 10), fr(89, 11),
             np.concatenate([piece(e, 2000, 100), tmr.rc(piece(e, 2300, 60))])]
    res = check_run(e, [reads], tmp_path)
    got = [(int(res["n"][i]), int(res["seqF"][i]), int(res["seqR"][i]), int(res["bad"][i]), int(res["isF"][i])) for i in range(len(reads))]
    assert got == [(99, 99, 0, 1, 0), (100, 100, 0, 0, 1), (100, 100, 0, 0, 1), (99, 0, 99, 1, 0), (100, 0, 100, 0, 0),
                   (100, 10, 90, 0, 0), (100, 11, 89, 1, 0), (22, 11, 11, 1, 0), (100, 50, 50, 1, 0), (100, 90, 10, 0, 1), (100, 89, 11, 1, 0),
                   (100, 100, 0, 0, 1)]


# ---- 4: -R's fatal cases ----

@pytest.mark.gpu
def test_fatal_cases(golden_dir, tmp_path):
    """two records; a stretch repeated; a mod at position 0 twice (accepted, the second position kept); the same mod three times"""
    L = mg.lib()
    rec = json.load(open(os.path.join(golden_dir, "rep_errors.json")))
    ref_mod = tmr.golden_paths(golden_dir, "k19d8")[1]
    p, rs = tmr.load_set(ref_mod)
    tmr.destroy_set(p)
    for name, want in rec.items():
        ref = L.mgRepRefCreate(os.path.join(golden_dir, name).encode(), ref_mod.encode(), None)
        if want["fatal"]:
            assert not ref and "FATAL ERROR: " + L.mgLastError().decode() == want["fatal"], name
            continue
        assert ref, (name, L.mgLastError())
        L.mgRepRefDestroy(ref)
        ref = mg.rep_ref_create(os.path.join(golden_dir, name), ref_mod, str(tmp_path / "e"))
        assert read_text(tmp_path / "e") == want["stderr"]
        seq = mg.fasta.read_fasta_list(os.path.join(golden_dir, name))[0]
        kmer, loc, _ = rs.h.scan(seq)
        x = int(rs.find(kmer[:1])[0])
        assert name == "rep_zero_twice.fa" and x and loc[0] == 0 and ref.contents.pos[x] == int(loc[rs.find(kmer) == x][-1]) > 0
        L.mgRepRefDestroy(ref)
    assert not L.mgRepRefCreate(b"/nonexistent/ref.fa", ref_mod.encode(), None) and L.mgLastError().decode() == "can't open reference sequence file /nonexistent/ref.fa"
    assert not L.mgRepRefCreate(os.path.join(golden_dir, "rep_two_seq.fa").encode(), b"/nonexistent/x.mod", None) and L.mgLastError().decode() == "failed to open mod file /nonexistent/x.mod"


# ---- 5: a file in batches ----

@pytest.mark.gpu
def test_batches(golden_dir, tmp_path):
    """the fixture's reads through one mgRepRunAdd, and through three whose cuts fall inside the run of bad reads and just behind a flipped
    read: the same lines (the read numbers go on across the calls) and the same arrays"""
    L = mg.lib()
    w = tmr.world(golden_dir, "k19d8")
    ref_fa, ref_mod, _, reads_mod = tmr.golden_paths(golden_dir, "k19d8")
    ref = mg.rep_ref_create(ref_fa, ref_mod)
    p_ms, _ = tmr.load_set(reads_mod)
    reads, no = w["reads"], {n: i for i, n in enumerate(w["names"])}
    cut1, cut2 = no["chimera"], no["fwd_then_rev"] + 1
    assert w["res"]["bad"][cut1 - 1] and w["res"]["bad"][cut1] and not w["res"]["bad"][cut2 - 1] and not w["res"]["isF"][cut2 - 1]
    one = run(ref, p_ms, [reads], tmp_path, "one")
    three = run(ref, p_ms, [reads[:cut1], reads[cut1:cut2], reads[cut2:]], tmp_path, "three")
    assert one[0] == three[0] == util.golden_text("rep_k19d8.stdout.txt")
    assert one[1] == three[1] == w["err"]
    tmr.results_equal(one[2], w["res"]); tmr.results_equal(three[2], w["res"])
    tmr.destroy_set(p_ms)
    L.mgRepRefDestroy(ref)


# ---- 6: tile edges ----

def reads_with_hits(e, total, first=0):
    """reads that hold the genome's modimizers first .. first + total - 1 once each, 100 or more a read, every other one reverse-complemented"""
    reads, at, j = [], first, 0
    while total:
        c = total if total < 1300 else 1100 + 37 * (j % 5)
        if total - c < 100 and total != c:
            c = total - 100
        s = piece(e, at, c)
        reads.append(tmr.rc(s) if j & 1 else s)
        at += c; total -= c; j += 1
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("total", [SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 3])
def test_hit_counts_on_sort_tile_edges(total, tmp_path):
    e = edge_world()
    reads = reads_with_hits(e, total)
    res = check_run(e, [reads], tmp_path)
    assert res["hitStart"][-1] == total and res["nBad"] == 0 and res["nDup"] == 0 and res["minMax"] == 1


@pytest.mark.gpu
def test_duplicates_across_a_sort_tile(tmp_path):
    """the first SORT_TILE - 1 mods once each, then mod SORT_TILE twice: its two hits are elements SORT_TILE - 1 and SORT_TILE of the sorted
    order.  In ONE read they are a duplicate; in two reads they are not"""
    e = edge_world()
    below = reads_with_hits(e, SORT_TILE - 1)
    a = piece(e, SORT_TILE - 1, 200)
    res = check_run(e, [below + [np.concatenate([a, a])]], tmp_path)
    assert res["modNPre"][SORT_TILE] == 1 and res["modN"][SORT_TILE] == 0 and res["nDup"] == 200 and res["modN"][SORT_TILE - 1] == 1
    res = check_run(e, [below + [a, a]], tmp_path)
    assert res["modNPre"][SORT_TILE] == 0 and res["modN"][SORT_TILE] == 2 and res["nDup"] == 0 and res["minMax"] == 1


@pytest.mark.gpu
def test_more_than_1024_reads(tmp_path):
    """1100 reads of about 250 bases, a little over 100 hits each, in two batches: the per-read passes cross 1024"""
    e = edge_world()
    reads = [piece(e, (j * 7) % 5000, 104 + j % 9) for j in range(1100)]
    reads = [tmr.rc(s) if j % 3 == 1 else s for j, s in enumerate(reads)]
    reads[1050] = piece(e, 30, 99)                                               # a bad one behind the 1024th
    res = check_run(e, [reads[:1030], reads[1030:]], tmp_path)
    assert res["nRead"] == 1100 and res["nBad"] == 1 and max(len(s) for s in reads) < 330


@pytest.mark.gpu
def test_empty_runs(tmp_path):
    """no good read; no read at all; a second set without entries"""
    e = edge_world()
    junk = [synth.iid_bases(600, 31), synth.iid_bases(0, 1), piece(e, 40, 50)]
    res = check_run(e, [junk], tmp_path)
    assert res["nGood"] == 0 and res["nBad"] == 3 and res["minMax"] == 0
    res = check_run(e, [], tmp_path)
    assert res["nRead"] == 0 and res["nMod"] == e["rs"].max
    empty = mg.modsetCreate(mg.seqhashCreate(K, W, 17), 20)
    res = check_run(e, [[piece(e, 0, 150), tmr.rc(piece(e, 100, 150))]], tmp_path, ms=empty, rms=tmr.RepSet(K, W, 17, np.zeros(1, np.uint64)))
    assert res["nGood"] == 2 and res["max"] == 0 and res["nMod"] == 0 and res["hitStart"][-1] == 0 and res["minMax"] == 0


# ---- 6b: more modimizers than the first guess ----

@pytest.mark.gpu
def test_seed_lists_retry_when_the_guess_is_too_small(tmp_path):
    """mg_modrep.hip asks mgSeedsOfBatch for min (bases / w * 2 + 4096, bases + 16) seeds.  w = 3 is the smallest that can fall short: a
    run of a (one k-mer, a modimizer at every start, in neither set) holds a seed per base against two per three bases provided for.
      -R     the reference sequence carries a run of 60 000 a in its middle;
      vote   two reads of 60 000 a (BADREADs with n 0) among reads that vote, an empty one, one of k - 1 bases, one with too few hits;
      hits   a good read that ends in a run of 60 000 a: the oriented batch falls short too.
    Every call goes round again; pos / isF / len, the lines and the result arrays against the restatement.  Then the same reads with
    a second set of max == 0: no hits, the totals as the restatement gives them."""
    L = mg.lib()
    k, w, seed = 21, 3, 17
    h = tmr.pyoracle.Hasher(k, w, seed)
    assert len(h.scan(np.zeros(k, np.uint8))[0]) == 1                             # the k-mer of a run of a IS a modimizer: the run is all seeds
    guess = lambda total: min(total // w * 2 + 4096, total + 16)                  # mg_modrep.hip, mgRepSeedList
    seeds = lambda seqs: sum(len(h.scan(s)[0]) for s in seqs)
    g = synth.iid_bases(9000, 7300)
    poly = np.zeros(60_000, np.uint8)
    kmer = h.scan(g)[0]
    assert len(np.unique(kmer)) == len(kmer) and kmer.min() > 0                   # no repeated mod (-R would die), and the run's k-mer (value 0) is not among them
    ms = mg.modsetCreate(mg.seqhashCreate(k, w, seed), 20)
    assert mg.add_sequence_batch(ms, *util.concat_reads([g])) == len(kmer)
    mg.check(L.modsetSyncToHost(ms, 0))
    rs = tmr.set_of(ms)
    # -R
    ref_seq = np.concatenate([g[:4000], poly, g[4000:]])
    assert guess(len(ref_seq)) < seeds([ref_seq]) <= len(ref_seq)
    rref = tmr.ref_create(rs, ref_seq)
    ref = mg.rep_ref_from_arrays(ms, ref_seq, str(tmp_path / "R.err"))
    r, m = ref.contents, rs.max
    assert read_text(tmp_path / "R.err") == rref["line"] and r.len == rref["len"]
    assert np.array_equal(np.ctypeslib.as_array(r.pos, (m + 1,)), rref["pos"]) and np.array_equal(np.ctypeslib.as_array(r.isF, (m + 1,)).astype(np.uint8), rref["isF"])
    # -s3
    reads = [g[:600], poly, tmr.rc(g[1000:1700]), g[:0], g[3000:3000 + k - 1], poly, g[2000:2200], np.concatenate([g[5000:5600], poly]), tmr.rc(g[6000:6500])]
    total = sum(len(s) for s in reads)
    assert guess(total) < seeds(reads) <= total                                   # the vote's batch
    e = dict(ref=ref, rs=rs, rref=rref, ms=ms)
    res = check_run(e, [reads], tmp_path)
    assert res["bad"].tolist() == [0, 1, 0, 1, 1, 1, 1, 0, 0] and res["n"].tolist()[1] == res["n"].tolist()[5] == 0 and 0 < res["n"][6] < 100
    good = [tmr.rc(reads[i]) if not res["isF"][i] else reads[i] for i in res["goodI"]]
    assert guess(sum(len(s) for s in good)) < seeds(good)                         # the oriented batch
    assert res["isF"].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0] and res["hitStart"][-1] > 500
    print("first guesses %d %d %d, seeds %d %d %d" % (guess(len(ref_seq)), guess(total), guess(sum(len(s) for s in good)), seeds([ref_seq]), seeds(reads), seeds(good)))
    empty = mg.modsetCreate(mg.seqhashCreate(k, w, seed), 20)
    res = check_run(e, [reads], tmp_path, ms=empty, rms=tmr.RepSet(k, w, seed, np.zeros(1, np.uint64)))
    assert res["nGood"] == 4 and res["max"] == 0 and res["nMod"] == 0 and res["hitStart"][-1] == 0 and res["minMax"] == 0
    L.mgRepRefDestroy(ref); L.modsetDestroy(ms); L.modsetDestroy(empty)


# ---- 7: entry max and entry 0 ----

@pytest.mark.gpu
def test_entry_max_is_tallied_and_not_counted(tmp_path):
    """reads on the set's last entries: n[max] and nPre[max] are tallied, the three counts run over 0 .. max - 1, entry 0 included"""
    e = edge_world()
    m = e["rs"].max
    last = piece(e, m - 150, 150)
    res = check_run(e, [[last, np.concatenate([last, last])]], tmp_path)
    assert res["modN"][m] == 3 and res["modNPre"][m] == 1 and res["modN"][m - 1] == 0 and res["modNPre"][m - 1] == 1
    assert res["nDup"] == 149 and res["nMod"] + res["nDup"] == m and res["nMod"] == m - 149
    assert res["minMax"] == 3                                                     # every mod below max that the reads hold is a dup and zeroed; entry max is past the zeroing


# ---- 8: the example ----

@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_rep_example_runs_like_modrep(tag, golden_dir, tmp_path):
    """examples/rep_file.c = `modrep -R ref.fa ref.mod -s3 reads.fa reads.mod` on the library, from plain C"""
    exe = str(tmp_path / "rep_file")
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "rep_file.c"),
                        "-o", exe, "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + list(tmr.golden_paths(golden_dir, tag)), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    assert r.stdout == util.golden_text("rep_%s.stdout.txt" % tag)
    assert r.stderr == util.golden_text("rep_%s.stderr.txt" % tag)
