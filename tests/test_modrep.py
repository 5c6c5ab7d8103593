"""modrep -R / -s3 (refCreate, modrep.c:27-63; analyzeSequences3, modrep.c:170-268): a plain numpy restatement of both, built on the
oracle's CPU scan, against the reference program's own output (tests/golden/rep_*: make_golden_modrep.py), which the GPU tests
(test_gpu_modrep.py) then lean on; the names in header, library and binding; the example compiles."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import fasta
from oracle import pyoracle
from tests import util

TAGS = {"k19d8": (19, 8), "k16d4": (16, 4)}
VOTES, MIXED = 100, 10                  # modrep.c:197,204
NAMES = {"mgRepRefCreate": "MgRepRef *", "mgRepRefFromArrays": "MgRepRef *", "mgRepRefDestroy": "void ", "mgRepRunBegin": "MgRepRun *", "mgRepRunAdd": "int  ",
         "mgRepRunFinish": "int  ", "mgRepResultFree": "void ", "mgRepAnalyze3File": "int  ", "mgRepPath": "int  "}


class RepFatal(Exception):
    """what the program die ()s with"""


def rc(s):
    return (3 - np.asarray(s, np.uint8)[::-1]).astype(np.uint8)


# ---- the restatement ----

class RepSet:
    """a set as the two passes use it: its hasher (the oracle's) and `modsetIndexFind (ms, kmer, false)` over its entries 1 .. max"""

    def __init__(self, k, w, seed, values):
        self.k, self.w, self.seed = k, w, seed
        self.h = pyoracle.Hasher(k, w, seed)
        self.max = len(values) - 1
        v = np.asarray(values[1:], np.uint64)
        order = np.argsort(v, kind="stable")
        self.sorted, self.idx = v[order], (order + 1).astype(np.int64)

    def find(self, kmers):
        kmers = np.asarray(kmers, np.uint64)
        if not len(self.sorted) or not len(kmers):
            return np.zeros(len(kmers), np.int64)
        p = np.minimum(np.searchsorted(self.sorted, kmers), len(self.sorted) - 1)
        return np.where(self.sorted[p] == kmers, self.idx[p], 0)


def set_of(ms):
    """RepSet of a Modset* whose host arrays are current"""
    value, _, _ = mg.modset_arrays(ms)
    h = ms.contents.hasher.contents
    return RepSet(h.k, h.w, h.seed, value)


def load_set(path):
    """(Modset*, RepSet) of a .mod file, gzip or plain; destroy the Modset* with destroy_set"""
    L = mg.lib()
    f = L.mgFzOpen(path.encode(), b"r")
    assert f, path
    ms = L.modsetRead(f)
    mg._libc.fclose(f)
    return ms, set_of(ms)


def destroy_set(ms):
    sh = C.cast(ms.contents.hasher, C.c_void_p).value                     # (the field is a view into the struct that modsetDestroy frees)
    mg.lib().modsetDestroy(ms); mg.lib().mgSeqhashDestroy(C.cast(sh, C.POINTER(mg.Seqhash)))


def ref_create(rs, seq):
    """refCreate on one sequence: dict(pos, isF, len, line); RepFatal as the program dies (modrep.c:48)"""
    kmer, loc, isf = rs.h.scan(seq)
    ix = rs.find(kmer)
    pos, is_f = np.zeros(rs.max + 1, np.int32), np.zeros(rs.max + 1, np.uint8)
    n = top = 0
    for j in np.flatnonzero(ix):
        x = ix[j]
        if pos[x]:
            raise RepFatal("duplicate mod entry at position %d in ref" % loc[j])
        pos[x], is_f[x] = loc[j], isf[j]
        top = max(top, int(loc[j]) + 1)
        n += 1
    return dict(pos=pos, isF=is_f, len=top, line="found %d of %d locations in ref length %d\n" % (n, rs.max, len(seq)))


def ref_create_file(rs, path):
    seqs = fasta.read_fasta_list(path)
    ref = ref_create(rs, seqs[0])
    if len(seqs) > 1:
        raise RepFatal("multiple sequences in ref file - only one allowed")
    return ref


def analyze3(rs, ref, ms, reads):
    """analyzeSequences3 over `reads` (a list of uint8 arrays): (stdout text, stderr text, the arrays MgRepResult holds)"""
    out = []
    n_all, f_all, r_all, bad_all, isf_all = [], [], [], [], []
    good_i, good_len, hit_start, hit_k, hit_x = [], [], [0], [], []
    mod_n, mod_pre = np.zeros(ms.max + 1, np.int64), np.zeros(ms.max + 1, np.int64)
    for i, s in enumerate(reads):
        kmer, _, isf = rs.h.scan(s)
        ix = rs.find(kmer)
        first = np.flatnonzero(ix)[:VOTES]                                        # modrep.c:197: the loop ends when n reaches 100
        n = len(first)
        seq_f = int((isf[first] == ref["isF"][ix[first]]).sum())
        seq_r = n - seq_f
        bad = n < VOTES or (seq_f > MIXED and seq_r > MIXED)
        n_all.append(n); f_all.append(seq_f); r_all.append(seq_r); bad_all.append(int(bad))
        if bad:
            isf_all.append(0)
            out.append("BADREAD %5d len %5d n %d F %4d R %4d\n" % (i + 1, len(s), n, seq_f, seq_r))
            continue
        flip = seq_f < seq_r
        isf_all.append(int(not flip))
        if flip:
            s = rc(s)
        kmer, loc, _ = rs.h.scan(s)                                               # still the reference set's hasher (modrep.c:223)
        k = ms.find(kmer)
        sel = k > 0
        k, x = k[sel], loc[sel]
        np.add.at(mod_n, k, 1)
        u, c = np.unique(k, return_counts=True)
        mod_pre[u] += c - 1                                                       # modrep.c:229: the second and later occurrence in this read
        good_i.append(i); good_len.append(len(s)); hit_k.append(k); hit_x.append(x); hit_start.append(hit_start[-1] + len(k))
    m = ms.max                                                                    # modrep.c:238: i < ms->max
    dup = mod_pre[:m] != 0
    n_dup, t_dup, n_mod = int(dup.sum()), int(mod_pre[:m][dup].sum()), int(m - dup.sum())
    mod_n[:m][dup] = 0
    min_max = 0
    for k in hit_k:
        mx = int(mod_n[k].max()) if len(k) else 0
        if not min_max or mx < min_max:
            min_max = mx
    err = "read %d reads, %d bad, %d good: mods total %d good %d dup %d avdup %.1f\n" % (len(reads), sum(bad_all), len(good_i), m, n_mod, n_dup, t_dup / n_dup if n_dup else 0.)
    err += "minimum max for a read is %d\n" % min_max
    cat = lambda a: np.concatenate(a).astype(np.int32) if a else np.zeros(0, np.int32)
    res = dict(nRead=len(reads), nBad=sum(bad_all), nGood=len(good_i), max=m, nMod=n_mod, nDup=n_dup, tDup=t_dup, minMax=min_max,
               n=np.array(n_all, np.int32), seqF=np.array(f_all, np.int32), seqR=np.array(r_all, np.int32), bad=np.array(bad_all, np.uint8), isF=np.array(isf_all, np.uint8),
               modN=mod_n.astype(np.int32), modNPre=mod_pre.astype(np.int32), goodI=np.array(good_i, np.int32), goodLen=np.array(good_len, np.int32),
               hitStart=np.array(hit_start, np.int64), hitK=cat(hit_k), hitX=cat(hit_x))
    return "".join(out), err, res


def results_equal(got, want):
    """array for array, scalar for scalar"""
    assert sorted(got) == sorted(want)
    for key in want:
        if isinstance(want[key], np.ndarray):
            assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
        else:
            assert got[key] == want[key], (key, got[key], want[key])


# ---- helpers shared with the GPU tests ----

def golden_paths(golden_dir, tag):
    stem = os.path.join(golden_dir, "rep_%s" % tag)
    return stem + "_ref.fa", stem + "_ref.mod", stem + "_reads.fa", stem + "_reads.mod"


_worlds = {}


def world(golden_dir, tag):
    """the fixture of a tag, restated once: dict(rs, ms: RepSets; ref; reads, names; out, err, res of analyze3)"""
    if tag not in _worlds:
        ref_fa, ref_mod, reads_fa, reads_mod = golden_paths(golden_dir, tag)
        p_ref, rs = load_set(ref_mod)
        p_ms, ms = load_set(reads_mod)
        destroy_set(p_ref); destroy_set(p_ms)
        ref = ref_create_file(rs, ref_fa)
        names, bases, offs = fasta.read_fasta(reads_fa)
        reads = [bases[offs[i]:offs[i + 1]] for i in range(len(names))]
        out, err, res = analyze3(rs, ref, ms, reads)
        _worlds[tag] = dict(rs=rs, ms=ms, ref=ref, reads=reads, names=names, out=out, err=err, res=res)
    return _worlds[tag]


# ---- the tests ----

@pytest.mark.parametrize("tag", list(TAGS))
def test_restatement_vs_reference_program(tag, golden_dir):
    """the numpy restatement on the fixture's files: the program's stdout and stderr byte for byte, and its stderr for the two other orders
    of the same reads (the orphan first: a smaller minimum; the orphan last: 0)"""
    w = world(golden_dir, tag)
    assert (w["rs"].k, w["rs"].w, w["ms"].k, w["ms"].w) == TAGS[tag] * 2
    assert w["out"] == util.golden_text("rep_%s.stdout.txt" % tag)
    assert w["ref"]["line"] + w["err"] == util.golden_text("rep_%s.stderr.txt" % tag)
    moved = json.load(open(os.path.join(golden_dir, "rep_%s.reorder.json" % tag)))
    mins = {}
    for where in ("orphan_first", "orphan_last"):
        out, err, res = analyze3(w["rs"], w["ref"], w["ms"], [w["reads"][i] for i in moved[where]["order"]])
        assert out == moved[where]["stdout"] and w["ref"]["line"] + err == moved[where]["stderr"]
        mins[where] = res["minMax"]
    assert 0 == mins["orphan_last"] < mins["orphan_first"] < w["res"]["minMax"]


@pytest.mark.parametrize("tag", list(TAGS))
def test_fixture_holds_what_it_is_for(tag, golden_dir):
    """what the program's output does not show: a good, flipped read with forward votes; flipped and unflipped reads; the orphan good with
    no hit; a mod twice in one read; no read on entry max; entry 0 counted"""
    w = world(golden_dir, tag)
    res, no = w["res"], {n: i for i, n in enumerate(w["names"])}
    i = no["fwd_then_rev"]
    assert not res["bad"][i] and not res["isF"][i] and 0 < res["seqF"][i] <= MIXED < res["seqR"][i]
    good = res["bad"] == 0
    assert (res["isF"][good] == 1).any() and (res["isF"][good] == 0).any()
    g = list(res["goodI"]).index(no["orphan"])
    assert res["hitStart"][g] == res["hitStart"][g + 1] and res["n"][no["orphan"]] == VOTES
    assert res["nDup"] > 0 and res["tDup"] >= res["nDup"] and res["nMod"] + res["nDup"] == res["max"]
    assert res["modN"][res["max"]] == 0 and res["modNPre"][res["max"]] == 0 and not (res["hitK"] == res["max"]).any()
    assert res["goodLen"].tolist() == [len(w["reads"][i]) for i in res["goodI"]]


def test_restatement_fatal_cases(golden_dir):
    """-R's two ways to die, and the occurrence at position 0 that does not protect its entry (modrep.c:48)"""
    rec = json.load(open(os.path.join(golden_dir, "rep_errors.json")))
    p, rs = load_set(golden_paths(golden_dir, "k19d8")[1])
    destroy_set(p)
    for name, want in rec.items():
        try:
            line = ref_create_file(rs, os.path.join(golden_dir, name))["line"]
            assert want["fatal"] is None and line == want["stderr"], name
        except RepFatal as e:
            assert "FATAL ERROR: " + str(e) == want["fatal"], name
    assert rec["rep_zero_twice.fa"]["fatal"] is None and rec["rep_thrice.fa"]["fatal"] and rec["rep_two_seq.fa"]["fatal"] and rec["rep_dup_ref.fa"]["fatal"]


def test_names_in_header_library_and_binding():
    header = open(os.path.join(util.ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n, ret in NAMES.items():
        assert re.search(r"^%s%s \(" % (re.escape(ret), n), header, re.M), n
        assert n in mg.EXPORTS and hasattr(L, n), n
    for s in ("} MgRepRef ;", "} MgRepResult ;", "typedef struct MgRepRun MgRepRun ;"):
        assert s in header, s
    assert callable(mg.rep_ref_create) and callable(mg.rep_analyze3_file) and callable(mg.rep_run)
    assert L.mgRepPath() == -1 or L.mgRepPath() == 0
    assert "mg_modrep.o" in open(os.path.join(mg.CSRC, "Makefile")).read() and os.path.exists(os.path.join(mg.CSRC, "mg_modrep.hip"))      # built, and so in the source hash


def test_example_compiles(tmp_path):
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    mg.lib()
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "rep_file.c"),
                        "-o", str(tmp_path / "rep_file"), "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
