"""`composition` (composition.c:32-121 over seqIOopenRead (file, 0, true) / seqIOread, seqio.c:30-73,234-346): a plain restatement of the
program, record by record as it reads them, against its own output (tests/golden/comp_*: make_golden_composition.py), which the GPU tests
(test_gpu_composition.py) then lean on; isqrt (100 len) against the C double expression of the -l bins; the lenMin pair folded in random
groupings against the serial rule; the names in header, library and binding; the example compiles."""
import glob
import itertools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util

GOLDEN = os.path.join(util.ROOT, "tests", "golden")
SUBSETS = ["".join(c) for r in range(4) for c in itertools.combinations("bql", r)]
FLAG = {"b": 1, "q": 2, "l": 4}
NAMES = {"mgCompositionFile": "int  ", "mgCompositionText": "int  ", "mgCompositionFree": "void ", "mgCompositionDiag": "void "}
KEPT = {ord(c): ord(c.upper()) for c in "ABCDGHKMNRSTVWYabcdghkmnrstvwy"}      # dna2textAmbigConv, seqio.c:621-630
KEPT[ord("-")] = ord("-")
MAXLEN = 1 << 31


def flags_of(subset):
    return sum(FLAG[c] for c in subset)


class Refused(Exception):
    """the program die()s, divides by zero or indexes a table out of bounds; .kind: 'rule' (args[0] = its words), 'byte' (.offset), 'div', 'open'"""
    def __init__(self, kind, msg, offset=None):
        Exception.__init__(self, msg)
        self.kind, self.offset = kind, offset


# ---- the reader: seqIOread, serially ----

def read_records(data):
    """(type, [(seq offset, seq bytes as in the file, qual offset, qual bytes or None)], stderr text): stops where the reader stops.
    Raises Refused ('rule') where it die()s.  FASTA sequences are the raw lines: convert () is the caller's"""
    n = len(data)
    if not n:
        raise Refused("open", "unreadable or empty")
    if data[0] not in b">@":
        raise Refused("open", "neither FASTA nor FASTQ")
    fastq = data[0] == ord("@")
    recs, line, pos = [], 1, 0

    def line_end(p, in_record_newline):
        """the newline that ends the line p is in; None where the reader runs out of bytes inside the record (bufAdvanceInRecord,
        seqio.c:215-219): no newline, or -- for the lines whose newline is stepped over inside the record -- a newline that is the last byte"""
        e = data.find(b"\n", p)
        if e < 0:
            return None, line
        if in_record_newline and e == n - 1:
            return None, line + 1
        return e, line

    while pos < n:
        if fastq and data[pos] != ord("@"):
            raise Refused("rule", "no initial @ for FASTQ record line %d" % line)
        e, at = line_end(pos, True)
        if e is None:
            return fastq, recs, "incomplete sequence record line %d\n" % at
        line += 1
        pos = e + 1
        if not fastq:
            start = pos
            while pos < n and data[pos] != ord(">"):
                e, at = line_end(pos, False)
                if e is None:
                    return fastq, recs, "incomplete sequence record line %d\n" % at
                line += 1
                pos = e + 1
            recs.append((start, data[start:pos], None, None))
            continue
        e, at = line_end(pos, True)
        if e is None:
            return fastq, recs, "incomplete sequence record line %d\n" % at
        seq_at, seq = pos, data[pos:e]
        line += 1
        pos = e + 1
        if data[pos] != ord("+"):
            raise Refused("rule", "missing + FASTQ line %d" % line)
        e, at = line_end(pos, True)
        if e is None:
            return fastq, recs, "incomplete sequence record line %d\n" % at
        line += 1
        pos = e + 1
        e, at = line_end(pos, False)
        if e is None:
            return fastq, recs, "incomplete sequence record line %d\n" % at
        if e - pos != len(seq):
            raise Refused("rule", "qual not same length as seq line %d" % line)
        recs.append((seq_at, seq, pos, data[pos:e]))
        line += 1
        pos = e + 1
    return fastq, recs, ""


def len_min_serial(lengths):
    """composition.c:64"""
    m = 0
    for n in lengths:
        if not m or n < m:
            m = n
    return m


def c_int(x):
    """an unsigned product as the program's int holds it"""
    x &= 0xffffffff
    return x - (1 << 32) if x >= 1 << 31 else x


def c_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def restate(data, flags):
    """(stdout, stderr, result dict) of `composition` with `flags` on the bytes `data`; raises Refused"""
    fastq, recs, err = read_records(data)
    base, qual = np.zeros(256, np.int64), np.zeros(256, np.int64)
    lengths = []
    for seq_at, seq, qual_at, q in recs:                  # per record, in the program's order: convert, -b, the length, -q
        s = np.frombuffer(seq, np.uint8)
        if not fastq:
            if (s >= 0x80).any():
                raise Refused("byte", "convert[] out of bounds", seq_at + int(np.argmax(s >= 0x80)))
            s = np.array([KEPT[c] for c in seq if c in KEPT], np.uint8)
        if flags & 1:
            if (s >= 0x80).any():
                raise Refused("byte", "totBase[] out of bounds", seq_at + int(np.argmax(s >= 0x80)))
            base += np.bincount(s, minlength=256)
        if len(s) >= MAXLEN:
            raise Refused("long", "a record of 2^31 bases or more")
        lengths.append(len(s))
        if flags & 2 and fastq:
            qq = np.frombuffer(q, np.uint8)
            bad = (qq < 33) | (qq >= 0x80)
            if bad.any():
                raise Refused("byte", "totQual[] out of bounds", qual_at + int(np.argmax(bad)))
            qual += np.bincount(qq - 33, minlength=256)
    n_seq, tot = len(lengths), sum(lengths)
    len_min, len_max = len_min_serial(lengths), max(lengths, default=0)
    out = ["%s file, %d sequences >= 0, %d total, %s average, %d min, %d max\n"
           % ("fastq" if fastq else "fasta", n_seq, tot, "%.2f" % (tot / n_seq) if n_seq else "-nan", len_min, len_max)]
    if flags & 1:
        out.append("bases\n")
        unprint = 0
        for i in range(256):
            if base[i]:
                if 0x20 <= i < 0x7f:
                    out.append("  %c %d %4.1f %%\n" % (i, base[i], base[i] * 100.0 / tot))
                else:
                    unprint += int(base[i])
        if unprint:
            out.append(" unprintable %d %4.1f %%\n" % (unprint, unprint * 100.0 / tot))
    if flags & 2 and fastq:
        out.append("qualities\n")
        run = 0
        for i in range(256):
            run += int(qual[i])
            if qual[i]:
                out.append(" %3d %d %4.1f %% %5.1f %%\n" % (i, qual[i], qual[i] * 100.0 / tot, run * 100.0 / tot))
    bin_count, bin_sum = np.zeros(0, np.int32), np.zeros(0, np.uint64)
    if flags & 4 and lengths:
        bins = [math.isqrt(100 * n) for n in lengths]
        n_bins = max(bins) + 1
        bin_count, bin_sum = np.zeros(n_bins, np.int32), np.zeros(n_bins, np.uint64)
        for b, n in zip(bins, lengths):
            bin_count[b] += 1
            bin_sum[b] += np.uint64(n)
        if len_min < len_max:
            d = n_bins // 20
            if not d:
                raise Refused("div", "arrayMax / 20 is 0")
            i, tot50 = 0, 0
            while i < n_bins and tot50 < 0.5 * tot:
                tot50 += int(bin_sum[i])
                i += 1
            out.append("approximate N50 %d\n" % c_div(c_int(i * (i + 1)), 100))
            out.append("length distribution (quadratic bins)\n")
            s = 0
            for i in range(n_bins):
                s += int(bin_count[i])
                if s and not (n_bins - 1 - i) % d:
                    out.append("  %d\t%d\n" % (c_div(c_int(i * i), 100), s))
                    s = 0
    res = dict(type=2 if fastq else 1, nSeq=n_seq, totLen=tot, lenMin=len_min, lenMax=len_max, base=base.astype(np.uint64), qual=qual.astype(np.uint64),
               binCount=bin_count, binSum=bin_sum)
    return "".join(out), err, res


# ---- the goldens ----

def goldens():
    """[(json file's stem, input path, {subset: run})]"""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "comp_*.json"))):
        g = json.load(open(p))
        out.append((os.path.basename(p)[:-5], os.path.join(GOLDEN, g["input"]), g["runs"]))
    return out


def test_goldens_are_there():
    names = {g[0] for g in goldens()}
    assert {"comp_mixed_fa", "comp_empty_mid_fa", "comp_empty_end_fa", "comp_single_fa", "comp_equal_fa", "comp_long_fa", "comp_reads_fq", "comp_many_fq", "comp_crlf_fq",
            "comp_nonl_fa", "comp_hdr_end_fa", "comp_hdr_only_fa", "comp_hdr_nonl_fa", "comp_cut_seq_fq", "comp_cut_qual_fq", "comp_cut_hdr_fq", "comp_cut_only_fq",
            "comp_die_plus_fq", "comp_die_qual_fq", "comp_die_at_fq"} <= names
    for stem, path, runs in goldens():
        assert sorted(runs) == sorted(SUBSETS) or (stem == "comp_crlf_fq" and sorted(runs) == sorted(s for s in SUBSETS if "q" not in s)), stem
        assert os.path.getsize(path) < 100000


@pytest.mark.parametrize("stem,path,runs", goldens(), ids=[g[0] for g in goldens()])
def test_restatement_vs_reference_program(stem, path, runs):
    """the program's stdout, stderr and exit status under every recorded subset of -b -q -l, byte for byte"""
    data = open(path, "rb").read()
    for subset, run in runs.items():
        try:
            out, err, _ = restate(data, flags_of(subset))
            status = 0
        except Refused as r:
            assert r.kind == "rule", (stem, subset, r)
            out, err, status = "", "FATAL ERROR: %s\n" % r, 255
        assert (out, err, status) == (run["stdout"], run["stderr"], run["status"]), (stem, subset)


def test_fixtures_hold_what_they_are_for():
    g = {stem: (open(path, "rb").read(), runs) for stem, path, runs in goldens()}
    assert ", 100 min, 100 max" in g["comp_empty_mid_fa"][1][""]["stdout"] and ", 0 min, 150 max" in g["comp_empty_end_fa"][1][""]["stdout"]
    assert "-nan average" in g["comp_hdr_only_fa"][1]["l"]["stdout"] and g["comp_hdr_only_fa"][1][""]["stderr"] == "incomplete sequence record line 2\n"
    assert " unprintable 3 " in g["comp_crlf_fq"][1]["b"]["stdout"]
    assert "length distribution" not in g["comp_equal_fa"][1]["bql"]["stdout"] and "length distribution" in g["comp_mixed_fa"][1]["l"]["stdout"]
    q = g["comp_reads_fq"][1]["q"]["stdout"]
    assert "\n   0 " in q and "\n  93 " in q and b"\n+q1 some" in g["comp_reads_fq"][0] and b"\n\n+" in g["comp_reads_fq"][0]
    assert "qualities" not in g["comp_mixed_fa"][1]["bql"]["stdout"]
    m = g["comp_mixed_fa"][1]["b"]["stdout"]
    assert all("  %s " % c in m for c in "-ABCDGHKMNRSTVWY") and not re.search(r"^  [a-z0-9EFIJLOPQUXZ] ", m, re.M)
    assert len(g["comp_long_fa"][0]) > 8 * 4096 and len(g["comp_many_fq"][0]) > 8 * 4096


# ---- the two pieces of arithmetic the device does differently ----

def test_isqrt_is_the_programs_bin():
    """composition.c:66: i = 10.*sqrt((double)len), truncated, equals isqrt (100 len): checked where they could part, at every len at
    which 100 len passes a perfect square, and one either side, for bins up to 200000 (len up to 4e8) and at the top of the int range"""
    m = np.arange(1, 200001, dtype=np.int64)
    first = (m * m + 99) // 100                             # the least len with 100 len >= m^2
    for lens in (first - 1, first, first + 1, np.array([MAXLEN - 2, MAXLEN - 1], np.int64)):
        lens = lens[lens >= 0]
        c_double = np.floor(10.0 * np.sqrt(lens.astype(np.float64))).astype(np.int64)
        x = 100 * lens
        r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
        r = np.where(r * r > x, r - 1, r)
        r = np.where((r + 1) * (r + 1) <= x, r + 1, r)
        assert ((r * r <= x) & ((r + 1) * (r + 1) > x)).all()
        assert (c_double == r).all()
    assert all(math.isqrt(100 * n) == int(10.0 * math.sqrt(float(n))) for n in (0, 1, 3, 4, 99, 100, 101, 6000, MAXLEN - 1))


NONE = (1 << 64) - 1


def pair_of(lengths):
    e, m = 0, NONE
    for n in lengths:
        if not n:
            e, m = 1, NONE
        elif n < m:
            m = n
    return e, m


def pair_then(a, b):
    return (1, b[1]) if b[0] else (a[0], min(a[1], b[1]))


def test_len_min_pair_folds_in_any_grouping():
    """a run of records acts on lenMin as (holds an empty record, least length after the last empty one); the pairs of consecutive runs,
    combined in any bracketing, give the serial rule's answer"""
    rng = np.random.default_rng(64)
    for _ in range(3000):
        lengths = [int(x) for x in rng.choice([0, 0, 1, 2, 5, 100, 7, 3000], rng.integers(0, 14))]
        cuts = sorted(int(x) for x in rng.integers(0, len(lengths) + 1, rng.integers(0, 6)))
        parts = [pair_of(lengths[a:b]) for a, b in zip([0] + cuts, cuts + [len(lengths)])]
        while len(parts) > 1:                              # combine a random adjacent pair
            i = int(rng.integers(0, len(parts) - 1))
            parts[i:i + 2] = [pair_then(parts[i], parts[i + 1])]
        e, m = parts[0]
        assert (0 if m == NONE else m) == len_min_serial(lengths), lengths
        # ... and as the kernels fold a range: the last part with an empty record, the minimum from there on
        parts = [pair_of(lengths[a:b]) for a, b in zip([0] + cuts, cuts + [len(lengths)])]
        last = max([i for i, p in enumerate(parts) if p[0]], default=0)
        assert min(p[1] for p in parts[last:]) == m
    assert len_min_serial([5, 0, 100]) == 100 and len_min_serial([5, 3, 0]) == 0


def test_restatement_refuses_what_the_program_cannot_do():
    with pytest.raises(Refused) as r:
        restate(b">a\nAC\n>b\nACG\n", 4)
    assert r.value.kind == "div"
    assert restate(b">a\nAC\n>b\nACG\n", 3)[0].startswith("fasta file, 2 sequences")
    with pytest.raises(Refused) as r:
        restate(b">a\nAC\xe9T\n", 0)
    assert r.value.kind == "byte" and r.value.offset == 5
    assert restate(b">a\xe9\nACT\n", 7)[2]["totLen"] == 3            # in a header it is no base
    fq = b"@a\nAC\xe9T\n+\nII I\n"
    assert restate(fq, 4)[2]["totLen"] == 4
    with pytest.raises(Refused) as r:
        restate(fq, 1)
    assert r.value.offset == 5
    with pytest.raises(Refused) as r:
        restate(fq, 2)
    assert r.value.offset == 12
    for bad in (b"", b"ACGT\n", b"b123"):
        with pytest.raises(Refused) as r:
            restate(bad, 0)
        assert r.value.kind == "open"


# ---- names, example ----

def test_names_in_header_library_and_binding():
    header = open(os.path.join(util.ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n, ret in NAMES.items():
        assert re.search(r"^%s%s \(" % (re.escape(ret), n), header, re.M), n
        assert n in mg.EXPORTS and hasattr(L, n), n
    assert "} MgComposition ;" in header and all(re.search(r"^#define MG_COMP_%s %d$" % (k, v), header, re.M) for k, v in (("BASES", 1), ("QUALS", 2), ("LENGTHS", 4)))
    assert (mg.COMP_BASES, mg.COMP_QUALS, mg.COMP_LENGTHS) == (1, 2, 4)
    assert callable(mg.composition_file) and callable(mg.composition_text) and callable(mg.composition_diag)
    assert "mg_composition.o" in open(os.path.join(mg.CSRC, "Makefile")).read() and os.path.exists(os.path.join(mg.CSRC, "mg_composition.hip"))


def test_no_device_no_counts():
    """like every batch entry point: without a HIP device the call fails and says so; there is no host computation of the counts"""
    if mg.lib().mgDeviceCount() > 0:
        return
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.composition_file(os.path.join(GOLDEN, "comp_mixed.fa"), 7)
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.composition_text(b">a\nACGT\n", 1)


def example_binary(tmp_path):
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    mg.lib()
    exe = str(tmp_path / "composition_file")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "composition_file.c"),
                        "-o", exe, "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_example_compiles(tmp_path):
    example_binary(tmp_path)
