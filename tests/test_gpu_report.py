"""modutils -P (refpaint, modutils.c:260-273) and -d (reportDepths, modutils.c:65-77) on the GPU: mgRefPaintFile, mgRefPaint,
mgReportDepths against the reference program's own output (tests/golden/report_*, made by make_golden_report.py), against the
reference program run live (when oracle/_ref is there), against the per-read facade, and at config 2's size."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import fasta, synth
import util

pytestmark = pytest.mark.gpu
TAGS = list(util.MODUTILS_TAGS)
OTHERS = ("a", "b", "seed", "k15")
REF_MU = os.path.join(util.ROOT, "oracle", "_ref", "modutils_ref")


def gpath(name):
    return os.path.join(util.GOLDEN, name)


def check_text(text, name):
    """the golden text itself, or its digest (util.check_dump)"""
    util.check_dump(text, name)


def load_mod(path, tmp):
    """modsetRead of a .mod file (gzip as the reference's -w writes it, or plain)"""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    open(tmp, "wb").write(raw)
    with mg.CFile(tmp, "r") as f:
        return mg.lib().modsetRead(f)


def build_set(tag, state, tmp_path):
    """the set of `modutils -c B k w s -a reads.fa -a reads2.fa` in one of three states: 'pending' (built on the device, counts not
    synced), 'synced' (modsetSyncToHost), 'loaded' (written and read back: host arrays only, no device table)"""
    L = mg.lib()
    B, k, w, s = util.MODUTILS_TAGS[tag]
    sh = mg.seqhashCreate(k, w, s)
    ms = mg.modsetCreate(sh, B)
    with mg.CFile(str(tmp_path / "added.txt"), "w") as f:
        for fa in ("reads.fa", "reads2.fa"):
            assert L.mgAddSequenceFile(ms, gpath(fa).encode(), f) == 0
    if state == "synced":
        mg.check(L.modsetSyncToHost(ms, 1))
    elif state == "loaded":
        mg.check(L.modsetSyncToHost(ms, 1))
        p = str(tmp_path / "cur.mod")
        with mg.CFile(p, "w") as f:
            L.modsetWrite(ms, f)
        L.modsetDestroy(ms)
        with mg.CFile(p, "r") as f:
            ms = L.modsetRead(f)
        assert not L.mgModsetDeviceSlots(ms)
    return ms


def others_for(tag, tmp_path):
    return [load_mod(gpath("report_%s_%s.mod" % (tag, o)), str(tmp_path / ("o_%s.mod" % o))) for o in OTHERS]


def host_state(ms):
    m = ms.contents
    return m.max, mg.modset_arrays(ms)


@pytest.mark.parametrize("state", ["pending", "synced", "loaded"])
@pytest.mark.parametrize("tag", TAGS)
def test_paint_file_matches_reference(tag, state, tmp_path):
    L = mg.lib()
    ms = build_set(tag, state, tmp_path)
    for fa, gold in (("ref.fa", "report_%s.paint.txt" % tag), ("reads.fa", "report_%s.paint_reads.txt" % tag)):
        out = str(tmp_path / "paint.txt")
        mg.refpaint_file(ms, gpath(fa), out)
        check_text(open(out).read(), gold)
    L.modsetDestroy(ms)


@pytest.mark.parametrize("tag", TAGS)
def test_paint_in_memory_matches_reference(tag, tmp_path):
    L = mg.lib()
    ms = build_set(tag, "pending", tmp_path)
    names, bases, offs = fasta.read_fasta(gpath("reads.fa"))
    out = str(tmp_path / "paint.txt")
    mg.refpaint(ms, bases, offs, names, out)
    check_text(open(out).read(), "report_%s.paint_reads.txt" % tag)
    L.modsetDestroy(ms)


@pytest.mark.parametrize("state", ["pending", "synced", "loaded"])
@pytest.mark.parametrize("tag", TAGS)
def test_report_depths_matches_reference(tag, state, tmp_path):
    """-d against a.mod, b.mod, a set at another seed and one at k = 15 (values wider than 30 bits never reach that table)"""
    L = mg.lib()
    ms = build_set(tag, state, tmp_path)
    others = others_for(tag, tmp_path)
    before = [(o.contents.max, mg.modset_arrays(o)) for o in others]
    mx = ms.contents.max
    out = str(tmp_path / "depths.txt")
    mg.report_depths(ms, others, out)
    check_text(open(out).read(), "report_%s.depths.txt" % tag)
    # nothing changes: the current set (max, then values, depths and info once synced) and the others
    assert ms.contents.max == mx
    mg.check(L.modsetSyncToHost(ms, 1))
    _, (v, d, i) = host_state(ms)
    # twice in a row (the others' tables resident now) gives the same bytes
    mg.report_depths(ms, others, out + "2")
    assert open(out + "2").read() == open(out).read()
    mg.check(L.modsetSyncToHost(ms, 1))
    mx2, (v2, d2, i2) = host_state(ms)
    assert mx == mx2 and np.array_equal(v, v2) and np.array_equal(d, d2) and np.array_equal(i, i2)
    for o, (m0, arrs) in zip(others, before):
        assert o.contents.max == m0 and all(np.array_equal(a, b) for a, b in zip(arrs, mg.modset_arrays(o)))
    for o in others:
        mg.check(L.mgModsetDeviceRelease(o))
        L.modsetDestroy(o)
    L.modsetDestroy(ms)


def test_report_depths_no_others_and_example(tmp_path):
    """-d with no other set; and examples/paint_file.c: modutils -c B k w s -a reads.fa -a reads2.fa -P ref.fa [-d ... a.mod ...]"""
    tag = "k21d64"
    L = mg.lib()
    ms = build_set(tag, "pending", tmp_path)
    out = str(tmp_path / "d0.txt")
    mg.report_depths(ms, [], out)
    gold = [l.split("\t")[:4] for l in open(gpath("report_%s.depths.txt" % tag)).read().splitlines()]
    assert [l.split("\t") for l in open(out).read().splitlines()] == gold
    L.modsetDestroy(ms)

    exe = str(tmp_path / "paint_file")
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"),
                        os.path.join(util.ROOT, "examples", "paint_file.c"), "-o", exe, "-L", libdir, "-lmodgpu",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    B, k, w, s = util.MODUTILS_TAGS[tag]
    mods = []
    for o in OTHERS:                                           # the example reads .mod files as fzopen does: gzip or plain
        mods.append(gpath("report_%s_%s.mod" % (tag, o)))
    r = subprocess.run([exe, str(B), str(k), str(w), str(s), "-a", gpath("reads.fa"), "-a", gpath("reads2.fa"), "-P", gpath("reads.fa"),
                        "-d", str(tmp_path / "ex_depths.txt")] + mods, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    check_text(r.stdout, "report_%s.paint_reads.txt" % tag)
    check_text(open(tmp_path / "ex_depths.txt").read(), "report_%s.depths.txt" % tag)


def write_fastq(path, names, seqs):
    with open(path, "w") as f:
        for n, s in zip(names, seqs):
            f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def text_records(path):
    """(names, sequences as text) of a FASTA file, lines joined"""
    names, seqs = [], []
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith(">"):
            names.append(line[1:].split()[0]); seqs.append([])
        else:
            seqs[-1].append(line)
    return names, ["".join(s) for s in seqs]


@pytest.mark.parametrize("tag", ["k21d64", "k31d4"])
def test_paint_input_forms_identical(tag, tmp_path):
    """plain FASTA (device parser), .fa.gz (host parser) and FASTQ give the same lines"""
    L = mg.lib()
    ms = build_set(tag, "pending", tmp_path)
    names, seqs = text_records(gpath("reads.fa"))
    gz = str(tmp_path / "reads.fa.gz")
    with open(gpath("reads.fa"), "rb") as a, gzip.open(gz, "wb") as b:
        shutil.copyfileobj(a, b)
    fq = str(tmp_path / "reads.fq")
    write_fastq(fq, names, seqs)
    outs = []
    for src in (gpath("reads.fa"), gz, fq):
        out = str(tmp_path / ("p%d.txt" % len(outs)))
        mg.refpaint_file(ms, src, out)
        outs.append(open(out).read())
    assert outs[0] == outs[1] == outs[2]
    check_text(outs[0], "report_%s.paint_reads.txt" % tag)
    L.modsetDestroy(ms)


def facade_paint(ms, names, reads):
    """what modutils.c:262-270 prints, through the per-read facade: modRCiterator + host modsetIndexFind (after a sync)"""
    L = mg.lib()
    mg.check(L.modsetSyncToHost(ms, 1))
    dep = np.ctypeslib.as_array(ms.contents.depth, (ms.contents.max + 1,))
    out = []
    for n, r in zip(names, reads):
        out.append("painting %s length %d\n" % (n, len(r)))
        km, pos, _ = mg.iterate(ms.contents.hasher, r)
        for x, p in zip(km.tolist(), pos.tolist()):
            ix = L.modsetIndexFind(ms, x, 0)
            if ix:
                out.append("  %d\t%d\n" % (p, dep[ix]))
    return "".join(out)


def test_paint_edge_records(tmp_path):
    """records shorter than k, empty records, records either side of the iterator's 12 288-base crossover"""
    L = mg.lib()
    k, w = 21, 16
    sh = mg.seqhashCreate(k, w, 17)
    ms = mg.modsetCreate(sh, 22)
    genome = synth.iid_bases(60000, 71)
    reads = [genome[i:i + 3000] for i in range(0, 57000, 1500)]
    b, o = util.concat_reads(reads)
    mg.add_sequence_batch(ms, b, o)
    lens = [0, 5, k - 1, k, k + 1, 12287, 12288, 12289, 20000, 0, 1]
    names, recs = [], []
    for i, n in enumerate(lens):
        names.append("e%d_%d" % (i, n)); recs.append(genome[1000 * i: 1000 * i + n])
    bb, oo = util.concat_reads(recs)
    out = str(tmp_path / "mem.txt")
    mg.refpaint(ms, bb, oo, names, out)
    mem = open(out).read()
    fa = str(tmp_path / "edge.fa")
    fasta.write_fasta(fa, names, recs)
    mg.refpaint_file(ms, fa, str(tmp_path / "file.txt"))
    assert open(tmp_path / "file.txt").read() == mem
    assert mem == facade_paint(ms, names, recs)
    assert mem.count("painting ") == len(lens) and "painting e0_0 length 0\n" in mem
    L.modsetDestroy(ms)


def test_paint_retries_when_the_seed_guess_is_too_small(tmp_path):
    """mgRefPaintBatchDevice sizes its three seed arrays for min (bases / w * 2 + 4096, bases + 16) seeds and, for a batch with more, frees
    them and makes them again at the size the scan asked for.  With w = 2 the first term alone is the batch, so the guess is its cap and
    never short; w = 3 is the smallest that can fall short: records of a alone (one k-mer, a modimizer at every start) hold a seed per
    base against two per three bases provided for.  Two such records of 60 000, ordinary ones, an empty one and one of k - 1 bases
    between them; the lines against the per-read facade."""
    from oracle import pyoracle as po
    L = mg.lib()
    k, w, seed = 21, 3, 17
    assert len(po.Hasher(k, w, seed).scan(np.zeros(k, np.uint8))[0]) == 1       # the k-mer of a run of a IS a modimizer: the run is all seeds
    sh = mg.seqhashCreate(k, w, seed)
    ms = mg.modsetCreate(sh, 22)
    genome = synth.iid_bases(30000, 73)
    b, o = util.concat_reads([genome[i:i + 3000] for i in range(0, 27000, 1500)] + [np.zeros(200, np.uint8)])
    mg.add_sequence_batch(ms, b, o)
    poly = np.zeros(60_000, np.uint8)
    recs = [poly, genome[1000:3000], poly, genome[7000:7000 + k - 1], genome[:0], genome[5000:9000]]
    names = ["q%d_%d" % (i, len(r)) for i, r in enumerate(recs)]
    total = sum(len(r) for r in recs)
    guess = min(total // w * 2 + 4096, total + 16)                               # mg_report.hip, mgRefPaintBatchDevice
    bb, oo = util.concat_reads(recs)
    out = str(tmp_path / "mem.txt")
    mg.refpaint(ms, bb, oo, names, out)
    mem = open(out).read()
    lines = mem.count("\n") - len(recs)                                          # one line per seed that is in the set: no more than the batch's seeds
    print("first guess %d, seed lines of the batch %d" % (guess, lines))
    assert guess < lines <= total                                                # the first attempt was too small: the call went round again
    assert mem == facade_paint(ms, names, recs)
    assert mem.count("painting ") == len(recs) and "  59979\t180\n" in mem and len(set(l.split("\t")[1] for l in mem.splitlines() if l.startswith("  "))) > 2
    L.modsetDestroy(ms)


def test_saturated_depth_and_value_zero(tmp_path):
    """the all-a k-mer (value 0, printed "0" by %llx) counted past 65535 (saturated): both reports"""
    L = mg.lib()
    k = 21
    sh = mg.seqhashCreate(k, 1, 17)                           # w = 1: every k-mer is a modimizer
    ms = mg.modsetCreate(sh, 20)
    sh2 = mg.seqhashCreate(k, 1, 17)
    ms2 = mg.modsetCreate(sh2, 20)
    reads = [np.zeros(70000, np.uint8), np.array([1, 2, 3] * 20, np.uint8)]
    b, o = util.concat_reads(reads)
    mg.add_sequence_batch(ms, b, o)                           # counts pending on the device
    b2, o2 = util.concat_reads([np.zeros(40, np.uint8)])
    mg.add_sequence_batch(ms2, b2, o2)
    out = str(tmp_path / "p.txt")
    mg.refpaint(ms, np.zeros(30, np.uint8), np.array([0, 30], np.int64), ["polyA"], out)
    assert open(out).read() == "painting polyA length 30\n" + "".join("  %d\t65535\n" % p for p in range(10))
    mg.report_depths(ms, [ms2], str(tmp_path / "d.txt"))
    lines = open(tmp_path / "d.txt").read().splitlines()
    assert lines[0] == "MH\t0\t0\t65535\t20"
    assert len(lines) == ms.contents.max
    mg.check(L.modsetSyncToHost(ms, 1))
    v, d, _ = mg.modset_arrays(ms)
    assert v[1] == 0 and d[1] == 65535
    for ln, vv, dd in zip(lines[1:], v[2:], d[2:]):
        assert ln == "MH\t%x\t0\t%d\t0" % (vv, dd)
    L.modsetDestroy(ms); L.modsetDestroy(ms2)


# ---- live against the reference program ----------------------------------------------------------------------------------

def random_fasta(path, genome, n, lo, hi, rng, nrate=0.002, prefix="r"):
    names, seqs = [], []
    for i in range(n):
        L = int(rng.integers(lo, hi))
        st = int(rng.integers(0, len(genome) - L))
        s = np.array(list("ACGT"))[genome[st:st + L]]
        if rng.random() < 0.5:
            s = np.array(list("TGCA"))[genome[st:st + L][::-1]]
        s = s.copy()
        s[rng.random(L) < nrate] = "N"
        s[rng.random(L) < 0.01] = "a"
        names.append("%s%d" % (prefix, i)); seqs.append("".join(s))
    with open(path, "w") as f:
        for nm, s in zip(names, seqs):
            f.write(">%s some description\n" % nm)
            for j in range(0, len(s), 60):
                f.write(s[j:j + 60] + "\n")


@pytest.mark.skipif(not os.path.exists(REF_MU), reason="oracle/_ref/modutils_ref absent")
@pytest.mark.parametrize("seed,k,w,B", [(1, 21, 16, 20), (2, 17, 8, 20), (3, 27, 5, 21)])
def test_live_against_reference_program(seed, k, w, B, tmp_path):
    L = mg.lib()
    rng = np.random.default_rng(seed)
    genome = synth.iid_bases(30000, 100 + seed)
    random_fasta(str(tmp_path / "reads.fa"), genome, 150, 50, 2500, rng)
    random_fasta(str(tmp_path / "reads2.fa"), genome, 80, 50, 2500, rng, prefix="s")
    random_fasta(str(tmp_path / "ref.fa"), genome, 6, 1, 14000, rng, prefix="chr")

    def ref(*args):
        r = subprocess.run([REF_MU, "-o", "log.txt"] + list(args), capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-800:]
        return r.stdout
    base = ["-c", str(B), str(k), str(w), "17", "-a", "reads.fa"]
    want_paint = "".join(l for l in ref(*(base + ["-P", "ref.fa"])).splitlines(keepends=True) if not l.startswith("total resources"))
    ref("-c", str(B), str(k), str(w), "17", "-a", "reads2.fa", "-w", "o1.mod")
    ref("-c", "20", str(k - 4), str(w), "17", "-a", "reads2.fa", "-w", "o2.mod")
    for o in ("o1", "o2"):
        open(tmp_path / (o + ".plain"), "wb").write(gzip.open(tmp_path / (o + ".mod")).read())
    ref(*(base + ["-d", "depths.txt", "o1.plain", "o2.plain"]))
    want_depths = open(tmp_path / "depths.txt").read()

    sh = mg.seqhashCreate(k, w, 17)
    ms = mg.modsetCreate(sh, B)
    with mg.CFile(str(tmp_path / "added.txt"), "w") as f:
        assert L.mgAddSequenceFile(ms, str(tmp_path / "reads.fa").encode(), f) == 0
    mg.refpaint_file(ms, str(tmp_path / "ref.fa"), str(tmp_path / "paint.txt"))
    assert open(tmp_path / "paint.txt").read() == want_paint
    others = [load_mod(str(tmp_path / (o + ".mod")), str(tmp_path / (o + ".lib"))) for o in ("o1", "o2")]
    mg.report_depths(ms, others, str(tmp_path / "mine.txt"))
    assert open(tmp_path / "mine.txt").read() == want_depths
    for o in others:
        L.modsetDestroy(o)
    L.modsetDestroy(ms)


# ---- config 2's size -------------------------------------------------------------------------------------------------------

def device_block(L, total, genome_bases, plan_seed, err_seed):
    starts, offs, strands = synth.ont_read_plan(total, genome_bases, plan_seed, n50=20000, sigma=0.6, lo=500, hi=200000)
    tot = int(offs[-1])
    d_g = mg.DeviceBuffer(L.mgPackedWords(genome_bases) * 4)
    mg.check(L.mgSynthGenome(d_g.ptr, genome_bases, 12345, None))
    d_s = mg.DeviceBuffer.from_numpy(starts); d_of = mg.DeviceBuffer.from_numpy(offs); d_st = mg.DeviceBuffer.from_numpy(strands)
    d_r = mg.DeviceBuffer(L.mgPackedWords(tot) * 4)
    mg.check(L.mgSynthReads(d_g.ptr, genome_bases, d_s.ptr, d_of.ptr, d_st.ptr, len(starts), tot, 0.05, err_seed, d_r.ptr, None))
    mg.check(L.mgStreamSynchronize(None))
    d_g.free()
    return d_r, d_of, tot, len(starts)


def dec_len(x):
    x = x.astype(np.int64)
    return 1 + sum((x >= 10 ** i).astype(np.int64) for i in range(1, 10))


def hex_len(v):
    n = np.ones(len(v), np.int64)
    for i in range(1, 16):
        n += (v >> np.uint64(4 * i)) != 0
    return n


def test_full_size_config2(tmp_path):
    """config 2's set (10 Gbp, k=21 d=64, ~1.03e8 entries) -d against a second block of the same size: max lines and the byte total
    numpy computes from the host arrays, 1e5 sampled lines against host modsetIndexFind; -P on 1 Gbp of synthetic reference (its first
    333 Mbp the reads' genome): sampled records against the per-read facade"""
    L = mg.lib()
    k, w, bits = 21, 64, 30
    total, G = 10_000_000_000, 333_333_333
    sets = []
    for plan_seed, err_seed in ((1000, 777), (2000, 778)):
        d_r, d_of, tot, nr = device_block(L, total, G, plan_seed, err_seed)
        ms = mg.modsetCreate(mg.seqhashCreate(k, w, 17), bits)
        n = C.c_uint64()
        mg.check(L.mgAddReadsDevice(ms, d_r.ptr, tot, d_of.ptr, nr, C.byref(n), None))
        d_r.free(); d_of.free()
        sets.append(ms)
    ms, ms2 = sets
    mx = ms.contents.max
    assert mx > 90_000_000
    out = str(tmp_path / "depths.txt")
    mg.report_depths(ms, [ms2], out)                          # ms: counts still pending on the device
    mg.check(L.modsetSyncToHost(ms, 1)); mg.check(L.modsetSyncToHost(ms2, 1))
    v, d, info = mg.modset_arrays(ms)
    v2, d2, _ = mg.modset_arrays(ms2)
    order = np.argsort(v2[1:]); sv = v2[1:][order]
    at = np.searchsorted(sv, v[1:]); at[at >= len(sv)] = 0
    hit = sv[at] == v[1:]
    od = np.where(hit, d2[1:][order][at], 0)
    want_bytes = int((3 + hex_len(v[1:]) + 3 + dec_len(d[1:]) + 1 + dec_len(od) + 1).sum())
    assert os.path.getsize(out) == want_bytes
    buf = np.fromfile(out, np.uint8)
    nl = np.flatnonzero(buf == 10)
    assert len(nl) == mx
    rng = np.random.default_rng(5)
    for i in rng.choice(mx, 100_000, replace=False).tolist():
        a = nl[i - 1] + 1 if i else 0
        line = buf[a:nl[i]].tobytes().decode()
        e = i + 1
        ix = L.modsetIndexFind(ms2, int(v[e]), 0)
        assert line == "MH\t%x\t%d\t%d\t%d" % (v[e], info[e] & 3, d[e], d2[ix] if ix else 0), (i, line)
    del buf, nl
    L.modsetDestroy(ms2)

    # -P on 1 Gbp: 100 records of 10 Mbp; the genome prefix-consistent with the reads' (mgSynthGenome is per base)
    nb, rec = 1_000_000_000, 10_000_000
    d_g = mg.DeviceBuffer(L.mgPackedWords(nb) * 4)
    mg.check(L.mgSynthGenome(d_g.ptr, nb, 12345, None))
    d_b = mg.DeviceBuffer(nb)
    mg.check(L.mgUnpackDevice(d_g.ptr, nb, d_b.ptr, None))
    g = d_b.to_numpy(np.uint8, nb)
    d_g.free(); d_b.free()
    fa = str(tmp_path / "big.fa")
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(fa, "wb") as f:
        for r in range(nb // rec):
            f.write(b">c%d\n" % r)
            f.write(lut[g[r * rec:(r + 1) * rec]].tobytes() + b"\n")
    pout = str(tmp_path / "paint.txt")
    mg.refpaint_file(ms, fa, pout)
    text = open(pout).read()
    parts = text.split("painting ")[1:]
    assert len(parts) == nb // rec
    for r in (0, 17, 60):                                     # in the reads' genome, its end, beyond it
        want = facade_paint(ms, ["c%d" % r], [g[r * rec:(r + 1) * rec]])
        assert "painting " + parts[r] == want, r
    assert parts[0].count("\n") > 100_000 and parts[60].count("\n") < 1000       # beyond the reads' genome: chance hits only
    L.modsetDestroy(ms)
