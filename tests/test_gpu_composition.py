"""mgCompositionFile / mgCompositionText on the device (mg_composition.hip) against the reference program's own output (tests/golden/comp_*)
and against test_composition.py's restatement of it: every golden under every subset of -b -q -l at the default window and at windows of
one 4 KiB tile; the edges of the kernels' geometry (a thread takes 16 bytes, a wave 1 KiB, a tile 4 KiB); skew; random files; gzip; the
refusals; the example."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from tests import test_composition as tc

pytestmark = pytest.mark.gpu

ALL = list(range(8))
WINDOWS = [None, 4]                      # MODGPU_TEXT_WINDOW_KB: the parser's default; one tile a window


def run_text(data, flags, window_kb=None):
    with mg.knobs(TEXT_WINDOW_KB=window_kb):
        return mg.composition_text(data, flags)


def same_result(got, want, where):
    for k in ("type", "nSeq", "totLen", "lenMin", "lenMax"):
        assert int(got[k]) == int(want[k]), (where, k, got[k], want[k])
    for k in ("base", "qual", "binCount", "binSum"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (where, k)


def check(data, flag_sets=ALL, windows=WINDOWS, where=""):
    """the library on `data` == the restatement, lines and counts, under every flag set and window"""
    for flags in flag_sets:
        try:
            want = tc.restate(data, flags)
        except tc.Refused as r:
            want = r
        for kb in windows:
            if isinstance(want, tc.Refused):
                with pytest.raises(mg.ModgpuError):
                    run_text(data, flags, kb)
                continue
            out, err, res = run_text(data, flags, kb)
            assert (out, err) == want[:2], (where, flags, kb)
            same_result(res, want[2], (where, flags, kb))


# ---- goldens ----

@pytest.mark.parametrize("window_kb", WINDOWS)
@pytest.mark.parametrize("stem,path,runs", tc.goldens(), ids=[g[0] for g in tc.goldens()])
def test_goldens(stem, path, runs, window_kb, tmp_path):
    """every recorded subset of the three flags, byte for byte against the program's stdout and stderr; a die () is -1 with its words"""
    with mg.knobs(TEXT_WINDOW_KB=window_kb):
        for subset, run in runs.items():
            flags = tc.flags_of(subset)
            if run["status"]:
                with pytest.raises(mg.ModgpuError) as e:
                    mg.composition_file(path, flags)
                assert run["stderr"] == "FATAL ERROR: %s\n" % str(e.value).split("failed: ", 1)[1] and e.value.out == b"" and e.value.err == b""
                continue
            out, err, res = mg.composition_file(path, flags)
            assert (out, err) == (run["stdout"], run["stderr"]), (stem, subset)
            same_result(res, tc.restate(open(path, "rb").read(), flags)[2], (stem, subset))
            if window_kb and os.path.getsize(path) > 8192:
                d = mg.composition_diag()
                assert d["windows"] >= (os.path.getsize(path) + 4095) // 4096 and d["launches"] >= 4 * d["windows"]


# ---- the kernels' geometry ----

EDGES = [15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097]


@pytest.mark.parametrize("end", EDGES)
def test_line_ends_at_an_edge(end):
    """a line whose newline is byte `end` - 1, `end` or `end` + 1 of the file ... every line of the record in turn, both formats"""
    rng = np.random.default_rng(end)
    seq = lambda n: bytes(rng.choice(np.frombuffer(b"ACGTNacgt-RY", np.uint8), n).tobytes())
    tail_fa = b">next one\n" + seq(40) + b"\n>last\n\n"
    # FASTA: the header's newline at `end`; the first sequence line's newline at `end`
    if end > 1:
        check(b">" + b"h" * (end - 1) + b"\n" + seq(70) + b"\n" + seq(9) + b"\n" + tail_fa, [7], where=("fa header", end))
    check(b">h\n" + seq(end - 3) + b"\n" + seq(33) + b"\n" + tail_fa, [7], where=("fa line", end))
    # ... and "\n>" across it: the '>' at byte `end` + 1
    check(b">h\n" + seq(end - 3) + b"\n>x\n" + seq(20) + b"\n", [7], where=("fa start", end))
    fq = lambda s: bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), s).tobytes())
    qual = lambda s: bytes(rng.choice(np.frombuffer(b"!~~~~~~~5I", np.uint8), s).tobytes())
    tail_fq = b"@t\n" + fq(30) + b"\n+t\n" + qual(30) + b"\n@u\n\n+\n\n"
    n = end - 3
    if n >= 0:
        check(b"@h\n" + fq(n) + b"\n+\n" + qual(n) + b"\n" + tail_fq, [7], where=("fq seq line", end))
    if end > 1:
        check(b"@" + b"h" * (end - 1) + b"\n" + fq(21) + b"\n+\n" + qual(21) + b"\n" + tail_fq, [7], where=("fq header", end))
    n = (end - 5) // 2                                     # @h\n SEQ \n+\n QUAL \n: the record's last newline at 2 n + 6
    if n >= 0 and 2 * n + 5 == end:
        check(b"@h\n" + fq(n) + b"\n+\n" + qual(n) + b"\n" + tail_fq, [7], where=("fq record end", end))
    if end > 12:                                           # the '+' line padded so that its newline is byte `end`
        check(b"@h\n" + fq(5) + b"\n+" + b"p" * (end - 10) + b"\n" + qual(5) + b"\n" + tail_fq, [7], where=("fq plus line", end))


def test_newline_ends_a_window_and_a_record_starts_the_next():
    """4 KiB windows: byte 4095 is a newline, byte 4096 a '>' / an '@'"""
    rng = np.random.default_rng(4096)
    s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 9000).tobytes())
    fa = b">a\n" + s[:4092] + b"\n>b\n" + s[:5000] + b"\n"
    assert fa[4095:4097] == b"\n>"
    check(fa, [0, 7], where="fa")
    n = (4096 - 8) // 2                                    # @a\n SEQ \n+x\n QUAL \n: 2 n + 8 bytes
    fq = b"@a\n" + s[:n] + b"\n+x\n" + b"I" * n + b"\n@b\n" + s[:300] + b"\n+\n" + b"~" * 300 + b"\n"
    assert fq[4095:4097] == b"\n@"
    check(fq, [0, 7], where="fq")
    with mg.knobs(TEXT_WINDOW_KB=4):
        mg.composition_text(fq, 7)
        assert mg.composition_diag()["crossed"] == 0 and mg.composition_diag()["windows"] == 2


def test_one_record_open_across_five_windows():
    rng = np.random.default_rng(20000)
    s = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), 20000).tobytes())
    fa = b">one record of 20 kb\n" + b"".join(s[i:i + 100] + b"\n" for i in range(0, len(s), 100))
    check(fa, [7], where="20 kb")
    with mg.knobs(TEXT_WINDOW_KB=4):
        out, err, res = mg.composition_text(fa, 7)
        d = mg.composition_diag()
    assert res["nSeq"] == 1 and res["totLen"] == res["lenMin"] == res["lenMax"] == 20000 and err == ""
    assert d["windows"] >= 5 and d["crossed"] >= 1 and d["tiles"] == d["windows"]


def test_fastq_record_in_four_windows():
    """every line of the record in a window of its own (4 KiB windows)"""
    rng = np.random.default_rng(4)
    n = 4500
    s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())
    fq = b"@" + b"h" * 4200 + b"\n" + s + b"\n+" + b"p" * 4300 + b"\n" + bytes(rng.choice(np.frombuffer(b"!5I~", np.uint8), n).tobytes()) + b"\n@z\nAC\n+\n~~\n"
    nl = [i for i, c in enumerate(fq) if c == 10][:4]
    assert len({p // 4096 for p in nl}) == 4
    check(fq, [0, 7], where="four windows")
    with mg.knobs(TEXT_WINDOW_KB=4):
        mg.composition_text(fq, 7)
        assert mg.composition_diag()["crossed"] >= 3


# ---- skew ----

def test_one_base_one_quality():
    """64 KiB of one base in one record; qualities that are all '~': the counts are exact"""
    fa = b">polyA\n" + b"A" * 65536 + b"\n"
    for kb in WINDOWS:
        out, err, res = run_text(fa, 7, kb)
        assert res["base"][ord("A")] == 65536 and int(res["base"].sum()) == 65536 and res["lenMax"] == 65536
    check(fa, [1, 5], where="polyA")
    fq = b"".join(b"@r%d\n" % i + b"ACGT" * 64 + b"\n+\n" + b"~" * 256 + b"\n" for i in range(200))
    for kb in WINDOWS:
        out, err, res = run_text(fq, 3, kb)
        assert res["qual"][93] == 200 * 256 and int(res["qual"].sum()) == 200 * 256 and [int(res["base"][c]) for c in b"ACGT"] == [200 * 64] * 4
    check(fq, [3], where="all ~")


# ---- random files ----

def random_file(rng, fastq):
    n_rec = int(rng.integers(1, 9))
    lens = [int(rng.choice([0, 1, int(rng.integers(0, 40)), int(rng.integers(0, 6001))])) for _ in range(n_rec)]
    parts = []
    for i, n in enumerate(lens):
        name = b"r%d" % i + (b" " + b"d" * int(rng.integers(0, 60)) if rng.random() < 0.5 else b"")
        if fastq:
            s = bytes(rng.choice(np.frombuffer(b"ACGTNacgtn.*", np.uint8), n).tobytes())
            q = bytes(rng.choice(np.frombuffer(b"!\"#5II~~~~~~@+", np.uint8), n).tobytes())
            parts.append(b"@" + name + b"\n" + s + b"\n+" + (name if rng.random() < 0.3 else b"") + b"\n" + q + b"\n")
        else:
            s = bytes(rng.choice(np.frombuffer(b"ACGTNacgtnRYKMSWBDHV- x>@", np.uint8), n).tobytes())
            width = int(rng.integers(1, 200))
            body = b"".join(s[j:j + width] + b"\n" for j in range(0, n, width))
            if rng.random() < 0.3:
                body += b"\n"
            parts.append(b">" + name + b"\n" + body.replace(b"\n>", b"\nA"))      # a '>' that begins a line would be a record start
    data = b"".join(parts)
    cut = rng.random()
    if cut < 0.15:
        data = data[:-1]                                   # no final newline
    elif cut < 0.25:
        data = data[:int(rng.integers(1, len(data)))]      # cut anywhere
    return data


@pytest.mark.parametrize("seed", range(24))
def test_random_files(seed):
    """seeded shapes, both formats, lengths 0 to 6000, lines of random width, some cut off: all flag subsets, both windows"""
    rng = np.random.default_rng(1000 + seed)
    data = random_file(rng, fastq=bool(seed & 1))
    check(data, ALL, where=("seed", seed))


# ---- gzip ----

@pytest.mark.parametrize("name", ["comp_long.fa", "comp_many.fq"])
def test_gzip_input(name, tmp_path):
    plain = os.path.join(tc.GOLDEN, name)
    data = open(plain, "rb").read()
    gz = str(tmp_path / (name + ".gz"))
    with gzip.open(gz, "wb") as f:
        f.write(data)
    two = str(tmp_path / (name + ".two.gz"))                # two members: gzread reads them as one stream
    open(two, "wb").write(gzip.compress(data[:10000]) + gzip.compress(data[10000:]))
    for kb in WINDOWS:
        with mg.knobs(TEXT_WINDOW_KB=kb):
            want = mg.composition_file(plain, 7)
            for p in (gz, two):
                got = mg.composition_file(p, 7)
                assert got[:2] == want[:2]
                same_result(got[2], want[2], (name, kb, p))
    cut = str(tmp_path / (name + ".cut.gz"))               # an unfinished last record in a stream: inflated a second time, up to the cut
    open(cut, "wb").write(gzip.compress(data[:-7]))
    want = tc.restate(data[:-7], 7)
    for kb in WINDOWS:
        with mg.knobs(TEXT_WINDOW_KB=kb):
            got = mg.composition_file(cut, 7)
        assert got[:2] == want[:2] and got[1].startswith("incomplete sequence record line ")


# ---- refusals ----

def refused(data, flags, match, kb=None):
    with pytest.raises(mg.ModgpuError, match=match) as e:
        run_text(data, flags, kb)
    assert e.value.out == b"", (data[:40], flags)
    return e.value


@pytest.mark.parametrize("kb", WINDOWS)
def test_refusals(kb, tmp_path):
    good = b"@g\nACGT\n+\nIIII\n"
    pad = b"".join(b"@p%d\n" % i + b"ACGT" * 30 + b"\n+\n" + b"5" * 120 + b"\n" for i in range(40))      # the breach lies past the first tile
    n_pad = 160
    for flags in ALL:
        refused(pad + b"@a\nACGT\nIIII\n+\n", flags, "missing \\+ FASTQ line %d$" % (n_pad + 3), kb)
        refused(pad + b"@a\nACGT\n\nIIII\n", flags, "missing \\+ FASTQ line %d$" % (n_pad + 3), kb)
        refused(pad + b"@a\nACGT\n+\nIII\n" + good, flags, "qual not same length as seq line %d$" % (n_pad + 4), kb)
        refused(pad + b"@a\nACG\n+\nIIII\n" + b"@b\nACGT\n+\nIII\n", flags, "qual not same length as seq line %d$" % (n_pad + 4), kb)      # the sums agree again later: the first one counts
        refused(pad + b"a\nACGT\n+\nIIII\n", flags, "no initial @ for FASTQ record line %d$" % (n_pad + 1), kb)
        refused(pad + b"@a\nACGT\nX", flags, "missing \\+ FASTQ line %d$" % (n_pad + 3), kb)                  # dies before the file runs out
    # -l where every record is shorter than 4 bases and the lengths differ: the result is filled all the same
    e = refused(b">a\nAC\n>b\nACG\n", 4, "divides by zero", kb)
    assert e.result["nSeq"] == 2 and e.result["lenMin"] == 2 and e.result["lenMax"] == 3 and len(e.result["binCount"]) == 18
    assert run_text(b">a\nAC\n>b\nACG\n", 3, kb)[2]["totLen"] == 5 and run_text(b">a\nAC\n>b\nAC\n", 7, kb)[2]["lenMin"] == 2
    # bytes the reference indexes its tables out of bounds with: the offset is named; without the flag that touches the byte the file is fine
    fa = b">h\xe9\n" + b"ACGT" * 1200 + b"\nAC\xe9T\n>b\nACGT\n"
    for flags in ALL:
        refused(fa, flags, "offset %d " % fa.index(b"\xe9T"), kb)
    assert run_text(fa.replace(b"AC\xe9T", b"ACGT"), 7, kb)[2]["totLen"] == 4808       # in the header it is no base
    assert run_text(b">a\nACGT\n>b\nAC\xe9", 7, kb)[1] == "incomplete sequence record line 4\n"      # in a record that is dropped, too
    fq = pad + b"@a\nAC\xe9T\n+\nII I\n" + good
    off = len(pad)
    for flags in ALL:
        if flags & 1:
            refused(fq, flags, "offset %d " % (off + 5), kb)
        elif flags & 2:
            refused(fq, flags, "offset %d " % (off + 12), kb)
        else:
            assert run_text(fq, flags, kb)[2]["nSeq"] == 42
    refused(pad + b"@a\nACGT\n+\nII\x80I\n", 2, "offset %d " % (off + 12), kb)
    refused(fq + b"@z\nAC\nII\n", 1, "offset %d " % (off + 5), kb)                  # the byte's record comes before the broken rule's
    refused(pad + b"@z\nAC\n+\nI\n" + fq[off:], 3, "qual not same length", kb)      # ... and the other way round
    assert run_text(good + b"@a\nAC\xe9T\n+\nII", 3, kb)[2]["nSeq"] == 1            # in a record that is dropped
    # what mgSeqOpen refuses
    refused(b"ACGT\n", 0, "neither FASTA nor FASTQ", kb)
    refused(b"", 0, "empty", kb)
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    for p in (str(empty), str(tmp_path / "missing.fa")):
        with pytest.raises(mg.ModgpuError, match="empty|failed to open"):
            mg.composition_file(p, 0)


# ---- the example ----

def test_example_reproduces_a_golden(tmp_path):
    exe = tc.example_binary(tmp_path)
    for stem, path, runs in tc.goldens():
        if stem in ("comp_mixed_fa", "comp_reads_fq", "comp_cut_seq_fq"):
            r = subprocess.run([exe, path], capture_output=True)
            assert (r.returncode, r.stdout.decode("latin-1"), r.stderr.decode("latin-1")) == (0, runs["bql"]["stdout"], runs["bql"]["stderr"]), stem
