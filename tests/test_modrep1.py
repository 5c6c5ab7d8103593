"""modrep -s1 / -s2 (analyzeSequences1, modrep.c:272-489; analyzeSequences2, modrep.c:493-539): a plain restatement of both, built on the
oracle's CPU scan and on test_modrep.py's restatement of -R, against the reference program's own output (tests/golden/rep1_*:
make_golden_modrep1.py), which the GPU tests (test_gpu_modrep1.py) then lean on; the closed form of the order addHit leaves
(modrep.c:129-148) against a literal replay; the names in header, library and binding; the example compiles.

The restatement replays addHit entry by entry, as the program does: the device code does not (it computes the order in closed form), so
the two agree only if the closed form is right."""
import os
import re
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import fasta
from tests import util
from tests import test_modrep as tmr

BOUNDARY = (1, 961, 1951, 2961)         # modrep.c:493-496
NMOD_CALLS, BUILDS = 5, 4               # cleanMods at modrep.c:354,370,392,424,446; buildPrePost at :373,395,427,449
NAMES = {"mgRep1ResultFree": "void ", "mgRepRunFinish1": "int  ", "mgRepAnalyze1File": "int  ", "mgRepAnalyze1Hits": "int  ", "mgRepCount2": "int  ",
         "mgRepAnalyze2File": "int  ", "mgRep1Diag": "void "}
REFUSAL = "entry max of the second set occurs in a read, which modrep -s1 cannot represent"


class Rep1Refused(Exception):
    """a hit on entry max: the program indexes mods[ms->max] of an array of ms->max (modrep.c:288,343)"""


# ---- addHit: the literal replay, and the closed form ----

def add_hit(a, k, dx):
    """modrep.c:129-148 on a list of [k, n, x]"""
    for i, h in enumerate(a):
        if h[0] == k:
            h[1] += 1
            h[2] += dx
            if i and h[1] > a[0][1]:
                a.insert(0, a.pop(i))
            return
    a.append([k, 1, dx])


def closed_form_order(partners):
    """the partners of one owner's list after its arrivals `partners` (in order), without replaying them.  c = the arrival's occurrence
    number within its partner; an arrival is a record when c exceeds every c before it in the list.  The records' c run 1, 2, 3, ..: the
    record of value v is the FIRST arrival with c == v.  Entries that ever made a record, latest record first, then the others by first arrival."""
    seen, first_with_c = {}, {}
    c_of = []
    for t, p in enumerate(partners):
        seen[p] = seen.get(p, 0) + 1
        c_of.append(seen[p])
        first_with_c.setdefault(seen[p], t)
    last_record, first_arrival = {}, {}
    for t, p in enumerate(partners):
        first_arrival.setdefault(p, t)
        if first_with_c[c_of[t]] == t:
            last_record[p] = t
    with_record = sorted(last_record, key=lambda p: -last_record[p])
    return with_record + sorted((p for p in first_arrival if p not in last_record), key=lambda p: first_arrival[p])


def closed_form_front(partners):
    """the largest final count; ties to the entry whose last arrival came first"""
    count, last = {}, {}
    for t, p in enumerate(partners):
        count[p] = count.get(p, 0) + 1
        last[p] = t
    return min(count, key=lambda p: (-count[p], last[p]))


# ---- the restatement: the end of the file (modrep.c:354-480) on hit lists ----

def c_div(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def analyze1_end(m, K, read_i, hits):
    """`hits`: per good read (k list, x list).  (stdout text, stderr text, the arrays MgRep1Result holds, diag dict)"""
    for k, _ in hits:
        if any(int(v) == m for v in k):
            raise Rep1Refused(REFUSAL)
    reads = [[int(i), [int(v) for v in k], [int(v) for v in x]] for i, (k, x) in zip(read_i, hits)]
    n = [0] * (m + 1)
    for _, k, _ in reads:
        for v in k:
            n[v] += 1
    n_pre, n_post = [0] * (m + 1), [0] * (m + 1)
    pre, post = [[] for _ in range(m + 1)], [[] for _ in range(m + 1)]
    slot0 = [(0, 0, 0)] * (m + 1)              # what arrp (mods[i].pre, 0, Hit) holds: arrayCreate clears, arrayMax = 0 does not
    out, nmod = [], []
    diag = dict(builds=0, links=0, entries=0, runs=0, dropped=0, stale=0)

    def clean():                                # modrep.c:97-127
        thresh = len(reads) // 2
        c = [0, 0, 0, 0]
        for i in range(m):
            if not n[i]:
                c[0] += 1
            elif n[i] < 5:
                n[i] = 0; c[1] += 1
            elif n[i] > thresh:
                n[i] = 0; c[2] += 1
            else:
                c[3] += 1
        out.append("NMOD mod0 %d modSmall %d modBig %d modGood %d\n" % tuple(c))
        nmod.append(c)
        for r in reads:
            keep = [j for j, v in enumerate(r[1]) if n[v]]
            r[1], r[2] = [r[1][j] for j in keep], [r[2][j] for j in keep]

    def build():                                # modrep.c:150-168
        links = 0
        for i in range(m + 1):
            pre[i], post[i], n_pre[i], n_post[i] = [], [], 0, 0
        for _, k, x in reads:
            for j in range(1, len(k)):
                dx = x[j] - x[j - 1]
                add_hit(post[k[j - 1]], k[j], dx); n_post[k[j - 1]] += 1
                add_hit(pre[k[j]], k[j - 1], dx); n_pre[k[j]] += 1
                links += 1
        for i in range(m + 1):
            if pre[i]:
                slot0[i] = tuple(pre[i][0])
        diag["builds"] += 1
        diag["links"] = max(diag["links"], links)
        diag["entries"] = max(diag["entries"], sum(len(a) for a in post))

    def verdicts():                             # modrep.c:374-391
        zero = []
        for i in range(m):
            if not n[i]:
                continue
            h = slot0[i]
            if not pre[i] and h[1]:
                diag["stale"] += 1
            if h[1] == n[i] and h[1] == n_post[h[0]]:
                zero.append(i)
                continue
            thr = n[i] // 2
            ok = any(e[1] >= 5 and (e[1] > thr or e[1] > n_post[e[0]] // 2) for e in pre[i]) \
                or any(e[1] >= 5 and (e[1] > thr or e[1] > n_pre[e[0]] // 2) for e in post[i])
            if not ok:
                zero.append(i)
        for i in zero:                          # (the tests read n[i] of the mod itself and nPre / nPost of others: order free)
            n[i] = 0

    clean()
    for r in reads:                             # modrep.c:356-369
        x_next, keep = 0, []
        for j, x in enumerate(r[2]):
            if x >= x_next:
                keep.append(j); x_next = x + K
            else:
                n[r[1][j]] -= 1; diag["runs"] += 1
        r[1], r[2] = [r[1][j] for j in keep], [r[2][j] for j in keep]
    clean()
    build(); verdicts(); clean()
    build()
    before = len(reads)
    kept = []
    for r in reads:                             # modrep.c:395-415
        weak = False
        for j in range(1, len(r[1])):
            e = [e for e in post[r[1][j - 1]] if e[0] == r[1][j]]
            assert len(e) == 1
            if e[0][1] < 5:
                weak = True
                break
        if not weak:
            kept.append(r)
    reads = kept
    diag["dropped"] = before - len(reads)
    err = "reduced %d reads to %d reads\n" % (before, len(reads))
    for i in range(m + 1):
        n[i] = 0
    for r in reads:                             # modrep.c:417-423: every hit but the last
        for v in r[1][:-1]:
            n[v] += 1
    clean()
    build(); verdicts(); clean()
    build()
    for i in range(m):                          # modrep.c:450-461
        if n[i]:
            out.append("MOD %d n %d pre %d (" % (i, n[i], n_pre[i]) + "".join(" %d:%d|%d:%d" % (e[0], e[1], n_post[e[0]], c_div(e[2], e[1])) for e in pre[i])
                       + ") post %d (" % n_post[i] + "".join(" %d:%d|%d:%d" % (e[0], e[1], n_pre[e[0]], c_div(e[2], e[1])) for e in post[i]) + ")\n")
    reads.sort(key=lambda r: r[1])              # readOrder: lexicographic on k, the shorter first on a common prefix; stable, as glibc's merge sort is
    block = 0
    for i, r in enumerate(reads):               # modrep.c:465-480: the last block's BLOCK line is never printed
        if i and r[1] != reads[i - 1][1]:
            out.append("BLOCK %3d" % block + "".join("\t%5d" % v for v in reads[i - 1][1]) + "\n")
            block = 0
        block += 1
        out.append("READ %5d n %3d mods" % (r[0], len(r[1])) + "".join("\t%5d" % v for v in r[1]) + "\n")

    def csr(lists):
        start = np.zeros(m + 2, np.int64)
        start[1:] = np.cumsum([len(a) for a in lists])
        flat = [e for a in lists for e in a]
        col = lambda j: np.array([e[j] for e in flat], np.int32)
        return start, col(0), col(1), col(2)
    pre_s, pre_k, pre_n, pre_x = csr(pre)
    post_s, post_k, post_n, post_x = csr(post)
    hs = np.zeros(len(reads) + 1, np.int64)
    hs[1:] = np.cumsum([len(r[1]) for r in reads])
    res = dict(max=m, nmod=np.array(nmod, np.int32), readsBefore=before, readsAfter=len(reads),
               modN=np.array(n, np.int32), modNPre=np.array(n_pre, np.int32), modNPost=np.array(n_post, np.int32),
               preStart=pre_s, preK=pre_k, preN=pre_n, preX=pre_x, postStart=post_s, postK=post_k, postN=post_n, postX=post_x,
               readI=np.array([r[0] for r in reads], np.int32), hitStart=hs, hitK=np.array([v for r in reads for v in r[1]], np.int32))
    return "".join(out), err, res, diag


def oriented_hits(rs, ref, ms, reads):
    """the per-read pass of -s1 (modrep.c:293-349): -s3's vote and orientation without the BADREAD lines; (nRead, nBad, read_i, hits)"""
    read_i, hits, n_bad = [], [], 0
    for i, s in enumerate(reads):
        kmer, _, isf = rs.h.scan(s)
        ix = rs.find(kmer)
        first = np.flatnonzero(ix)[:tmr.VOTES]
        seq_f = int((isf[first] == ref["isF"][ix[first]]).sum())
        seq_r = len(first) - seq_f
        if len(first) < tmr.VOTES or (seq_f > tmr.MIXED and seq_r > tmr.MIXED):
            n_bad += 1
            continue
        if seq_f < seq_r:
            s = tmr.rc(s)
        kmer, loc, _ = rs.h.scan(s)
        k = ms.find(kmer)
        read_i.append(i); hits.append((k[k > 0], loc[k > 0]))
    return len(reads), n_bad, read_i, hits


def analyze1(rs, ref, ms, reads):
    """analyzeSequences1 over `reads`: (stdout, stderr, result arrays, diag)"""
    n_read, n_bad, read_i, hits = oriented_hits(rs, ref, ms, reads)
    out, err, res, diag = analyze1_end(ms.max, rs.k, read_i, hits)
    res.update(nRead=n_read, nBad=n_bad, nGood=len(read_i))
    return out, "read %d reads, %d bad, %d good: \n" % (n_read, n_bad, len(read_i)) + err, res, diag


def count2(rs, reads):
    """analyzeSequences2's four counts (modrep.c:519-535): the reads as they are, the reference set's hasher and entries"""
    c = [0, 0, 0, 0]
    for s in reads:
        ix = rs.find(rs.h.scan(s)[0])
        has = [bool((ix == b).any()) for b in BOUNDARY]
        for j in range(4):
            c[j] += has[j] and has[(j + 1) % 4]
    return c


# ---- helpers shared with the GPU tests ----

def golden_paths(golden_dir):
    ref_fa, ref_mod, _, _ = tmr.golden_paths(golden_dir, "k19d8")
    return ref_fa, ref_mod, os.path.join(golden_dir, "rep1_reads.fa"), os.path.join(golden_dir, "rep1_reads.mod")


_world = {}


def world(golden_dir):
    """the fixture restated once: dict(rs, ms, ref, reads, names; out1, err1, res1, diag1; counts2)"""
    if not _world:
        ref_fa, ref_mod, reads_fa, reads_mod = golden_paths(golden_dir)
        p_ref, rs = tmr.load_set(ref_mod)
        p_ms, ms = tmr.load_set(reads_mod)
        tmr.destroy_set(p_ref); tmr.destroy_set(p_ms)
        ref = tmr.ref_create_file(rs, ref_fa)
        names, bases, offs = fasta.read_fasta(reads_fa)
        reads = [bases[offs[i]:offs[i + 1]] for i in range(len(names))]
        out1, err1, res1, diag1 = analyze1(rs, ref, ms, reads)
        _world.update(rs=rs, ms=ms, ref=ref, reads=reads, names=names, out1=out1, err1=err1, res1=res1, diag1=diag1, counts2=count2(rs, reads))
    return _world


# ---- the tests ----

def test_restatement_vs_reference_program(golden_dir):
    """(a) the restatement on the fixture's files: the program's stdout and stderr for `-R .. -s1 .. -s2 ..`, byte for byte"""
    w = world(golden_dir)
    assert w["rs"].max > BOUNDARY[3]
    out = w["out1"] + "n1 %d n2 %d n3 %d n4 %d\n" % tuple(w["counts2"])
    assert out == util.golden_text("rep1.stdout.txt")
    assert w["ref"]["line"] + w["err1"] == util.golden_text("rep1.stderr.txt")
    assert len(w["res1"]["nmod"]) == NMOD_CALLS and w["diag1"]["builds"] == BUILDS


def test_fixture_holds_what_it_is_for(golden_dir):
    """what make_golden_modrep1.py asserts from the program's output, seen from the restatement: pruning of every kind happened"""
    w = world(golden_dir)
    res, diag = w["res1"], w["diag1"]
    assert res["nGood"] >= 10 and 0 < res["readsAfter"] < res["readsBefore"] and diag["runs"] > 0 and diag["links"] > 0
    assert (np.diff(res["preStart"]) >= 2).any() and (np.diff(res["postStart"]) >= 2).any()
    assert min(w["counts2"]) > 0 and len(set(w["counts2"])) > 1
    n_read, n_bad, _, hits = oriented_hits(w["rs"], w["ref"], w["ms"], w["reads"])
    assert n_bad > 0 and not any((k == w["ms"].max).any() for k, _ in hits)      # a bad read; entry max in no read
    lists = [res["preK"][a:b].tolist() for a, b in zip(res["preStart"][:-1], res["preStart"][1:])]
    assert len(set(res["readI"].tolist())) == res["readsAfter"] and max(len(a) for a in lists) >= 2


def test_entry_max_fixture_is_refused(golden_dir):
    """the second file holds a read on entry max: the program does not finish cleanly (the fixture records only that); the restatement refuses"""
    w = world(golden_dir)
    p_ms, ms = tmr.load_set(os.path.join(golden_dir, "rep1_max_reads.mod"))
    tmr.destroy_set(p_ms)
    names, bases, offs = fasta.read_fasta(os.path.join(golden_dir, "rep1_max_reads.fa"))
    reads = [bases[offs[i]:offs[i + 1]] for i in range(len(names))]
    with pytest.raises(Rep1Refused):
        analyze1(w["rs"], w["ref"], ms, reads)
    assert "not finish cleanly" in util.golden_text("rep1_max.note.txt")


def test_closed_form_of_add_hit_order():
    """(b) 2 000 seeded random arrival sequences, 1-6 partners and 1-40 arrivals (ties are frequent): the full list order and the front"""
    rng = np.random.default_rng(20200619)
    moved = 0
    for _ in range(2000):
        partners = rng.integers(10, 10 + rng.integers(1, 7), size=rng.integers(1, 41)).tolist()
        a = []
        for p in partners:
            add_hit(a, p, 1)
        want = [e[0] for e in a]
        assert closed_form_order(partners) == want, partners
        assert closed_form_front(partners) == want[0], partners
        first = list(dict.fromkeys(partners))
        moved += want != first
        assert sorted(want) == sorted(first) and sum(e[1] for e in a) == len(partners)
    assert moved > 200                                                            # a move to the front is common in these


def test_names_in_header_library_and_binding():
    """(c)"""
    header = open(os.path.join(util.ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n, ret in NAMES.items():
        assert re.search(r"^%s%s \(" % (re.escape(ret), n), header, re.M), n
        assert n in mg.EXPORTS and hasattr(L, n), n
    assert "} MgRep1Result ;" in header
    assert callable(mg.rep_analyze1_file) and callable(mg.rep_analyze1_hits) and callable(mg.rep_analyze2_file) and callable(mg.rep_count2) and callable(mg.rep1_diag)
    assert "mg_modrep1.o" in open(os.path.join(mg.CSRC, "Makefile")).read() and os.path.exists(os.path.join(mg.CSRC, "mg_modrep1.hip"))
    assert os.path.exists(os.path.join(mg.CSRC, "mg_modrep_int.h"))


def test_example_compiles(tmp_path):
    """(d)"""
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    mg.lib()
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "rep1_file.c"),
                        "-o", str(tmp_path / "rep1_file"), "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
