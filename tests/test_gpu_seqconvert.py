"""mgSeqConvertFile / mgSeqConvertText on the device (mg_seqconvert.hip) against the reference programs' own output (tests/golden/conv_*) and
against test_seqconvert.py's restatement of them: every golden as FASTA, FASTQ and homopolymer-compressed at the default window and at
windows of one 4 KiB tile; the edges of the kernels' geometry (a thread takes 16 bytes, a wave 1 KiB, a tile 4 KiB); what MG_SEQ_HOCO and
the '!' lines of FASTA -> FASTQ carry from tile to tile and window to window; random files; gzip; the refusals; the example.  Nothing is
held against the library's own output."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import modimizer_amd as mg
from tests import test_seqconvert as ts

pytestmark = pytest.mark.gpu

FASTA, FASTQ, HOCO = ts.FASTA, ts.FASTQ, ts.HOCO
ALL = [FASTA, FASTQ, HOCO]
WINDOWS = [None, 4]                      # MODGPU_TEXT_WINDOW_KB: the parser's default; one tile a window
EDGES = [15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097]


def run_text(data, flags, window_kb=None):
    with mg.knobs(TEXT_WINDOW_KB=window_kb):
        return mg.seq_convert_text(data, flags)


def check(data, modes=ALL, windows=WINDOWS, where=""):
    """the library on `data` == the restatement: output, stderr and counters, in every mode and window; a refusal names the offset or has
    the program's words, and leaves no output"""
    for flags in modes:
        try:
            want = ts.restate(data, flags)
        except ts.Refused as r:
            want = r
        for kb in windows:
            if isinstance(want, ts.Refused):
                with pytest.raises(mg.ModgpuError) as e:
                    run_text(data, flags, kb)
                assert e.value.out == b"", (where, flags, kb)
                assert ("offset %d " % want.offset if want.kind == "byte" else str(want)) in str(e.value), (where, flags, kb, str(e.value), str(want))
                continue
            out, err, res = run_text(data, flags, kb)
            assert out == want[0], (where, flags, kb, first_difference(out, want[0]))
            assert err == want[1] and res == want[2], (where, flags, kb, err, res, want[2])


def first_difference(a, b):
    n = min(len(a), len(b))
    i = next((i for i in range(n) if a[i] != b[i]), n)
    return (len(a), len(b), i, a[max(0, i - 20):i + 20], b[max(0, i - 20):i + 20])


def seq(rng, n, alphabet=b"ACGTNacgt-RY"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).tobytes())


# ---- goldens ----

@pytest.mark.parametrize("window_kb", WINDOWS)
@pytest.mark.parametrize("stem,path,runs", ts.goldens(), ids=[g[0] for g in ts.goldens()])
def test_goldens(stem, path, runs, window_kb, tmp_path):
    """every recorded mode, byte for byte against the program's stdout (less the byte seqhoco appends to a line) and stderr; a die () is -1
    with its words and no file"""
    data = open(path, "rb").read()
    with mg.knobs(TEXT_WINDOW_KB=window_kb):
        for mode, run in runs.items():
            want_out, want_err = ts.expected_of(stem, mode, run)
            dst = str(tmp_path / ("out_" + mode))
            if want_out is None:
                with pytest.raises(mg.ModgpuError) as e:
                    mg.seq_convert_file(path, dst, ts.MODES[mode])
                assert str(e.value).split("failed: ", 1)[1] == want_err and e.value.err == b"" and not os.path.exists(dst), (stem, mode)
                continue
            err, res = mg.seq_convert_file(path, dst, ts.MODES[mode])
            assert (open(dst, "rb").read(), err) == (want_out, want_err), (stem, mode)
            assert res == ts.restate(data, ts.MODES[mode])[2], (stem, mode)
            d = mg.seq_convert_diag()
            assert d["launches"] > 0 and d["windows"] >= 1
            if window_kb:
                assert d["windows"] >= (len(data) + 4095) // 4096 and d["tiles"] == d["windows"], (stem, mode, d)


# ---- the kernels' geometry ----

@pytest.mark.parametrize("end", EDGES)
def test_boundaries_at_an_edge(end):
    """the id's separator, the header's newline, a sequence line's newline, the record's end, the '+' line and the last quality byte at
    byte `end` of the text, both formats"""
    rng = np.random.default_rng(end)
    tail_fa = b">next one\n" + seq(rng, 40) + b"\n>last  d\n\n"
    fq = lambda n: seq(rng, n, b"ACGTNacgtn")
    qual = lambda n: seq(rng, n, b"!~~~~~~~5I@+")
    tail_fq = b"@t x\n" + fq(30) + b"\n+t\n" + qual(30) + b"\n@u\n\n+\n\n"
    # FASTA: the separator at `end` (a tab, then a description that begins with a space); the header's newline; a line's newline; "\n>"
    check(b">" + b"i" * (end - 1) + b"\t some words\n" + seq(rng, 70) + b"\n" + tail_fa, where=("fa separator", end))
    check(b">" + b"i" * (end - 1) + b" \n" + seq(rng, 70) + b"\n" + tail_fa, where=("fa separator, no description", end))
    check(b">id " + b"d" * (end - 4) + b"\n" + seq(rng, 70) + b"\n" + seq(rng, 9) + b"\n" + tail_fa, where=("fa header", end))
    check(b">h\n" + seq(rng, end - 3) + b"\n" + seq(rng, 33) + b"\n" + tail_fa, where=("fa line", end))
    check(b">h\n" + seq(rng, end - 4) + b"\n>x y\n" + seq(rng, 20) + b"\n", where=("fa record end", end))
    check(b">h\n" + seq(rng, end - 3) + b"\n>x y\n" + seq(rng, 20) + b"\n", where=("fa record start", end))
    # FASTQ: the same, then the '+' line's first byte and newline, and the last quality byte
    check(b"@" + b"i" * (end - 1) + b"\t some words\n" + fq(21) + b"\n+\n" + qual(21) + b"\n" + tail_fq, where=("fq separator", end))
    check(b"@id " + b"d" * (end - 4) + b"\n" + fq(21) + b"\n+\n" + qual(21) + b"\n" + tail_fq, where=("fq header", end))
    n = end - 3
    check(b"@h\n" + fq(n) + b"\n+\n" + qual(n) + b"\n" + tail_fq, where=("fq seq line, '+' behind it", end))
    check(b"@h\n" + fq(5) + b"\n+" + b"p" * (end - 10) + b"\n" + qual(5) + b"\n" + tail_fq, where=("fq plus line", end))
    n, pad = (end - 6) // 2, b"x" * ((end - 6) % 2)          # @h\n SEQ \n+[x]\n QUAL \n: the last quality byte is byte `end`, the record's last newline behind it
    check(b"@h\n" + fq(n) + b"\n+" + pad + b"\n" + qual(n) + b"\n" + tail_fq, where=("fq record end", end))


def test_newline_ends_a_window_and_a_record_starts_the_next():
    rng = np.random.default_rng(4096)
    s = seq(rng, 9000, b"ACGT")
    fa = b">a\n" + s[:4092] + b"\n>b\n" + s[:5000] + b"\n"
    assert fa[4095:4097] == b"\n>"
    check(fa, where="fa")
    n = (4096 - 8) // 2
    fq = b"@a\n" + s[:n] + b"\n+x\n" + b"I" * n + b"\n@b\n" + s[:300] + b"\n+\n" + b"~" * 300 + b"\n"
    assert fq[4095:4097] == b"\n@"
    check(fq, where="fq")
    with mg.knobs(TEXT_WINDOW_KB=4):
        mg.seq_convert_text(fq, FASTA)
        assert mg.seq_convert_diag()["crossed"] == 0 and mg.seq_convert_diag()["windows"] == 4      # two walks


def test_one_record_open_across_five_windows():
    rng = np.random.default_rng(20000)
    s = seq(rng, 20000, b"ACGTacgtN")
    fa = b">one record of 20 kb\n" + b"".join(s[i:i + 100] + b"\n" for i in range(0, len(s), 100))
    check(fa, where="20 kb")
    with mg.knobs(TEXT_WINDOW_KB=4):
        out, err, res = mg.seq_convert_text(fa, FASTA)
        d = mg.seq_convert_diag()
    assert res["nSeq"] == 1 and res["totSeqLen"] == res["maxSeqLen"] == 20000 and err == ""
    assert d["windows"] >= 10 and d["crossed"] >= 8 and d["tiles"] == d["windows"]


def test_fastq_record_in_four_windows():
    """every line of the record in a window of its own (4 KiB windows)"""
    rng = np.random.default_rng(4)
    n = 4500
    fq = b"@" + b"h" * 2100 + b" " + b"d" * 2100 + b"\n" + seq(rng, n, b"ACGT") + b"\n+" + b"p" * 4300 + b"\n" + seq(rng, n, b"!5I~") + b"\n@z\nAC\n+\n~~\n"
    nl = [i for i, c in enumerate(fq) if c == 10][:4]
    assert len({p // 4096 for p in nl}) == 4
    check(fq, where="four windows")


def test_more_than_1024_tiles_in_a_window():
    """4.3 MB go through in one window of 8 MiB: the one-workgroup scans take two tiles a thread"""
    rng = np.random.default_rng(1024)
    reads = [seq(rng, int(n), b"ACGTacgtn") for n in rng.integers(0, 20000, 430)]
    fq = b"".join(b"@r%d len=%d\n" % (i, len(s)) + s + b"\n+\n" + seq(rng, len(s), b"!5I~@+") + b"\n" for i, s in enumerate(reads))
    fa = b"".join(b">r%d\tlen=%d\n" % (i, len(s)) + b"".join(s[j:j + 70] + b"\n" for j in range(0, len(s), 70)) for i, s in enumerate(reads))
    assert len(fq) > 1024 * 4096 * 2 and 1024 * 4096 < len(fa) < 8 << 20
    check(fq, [FASTA, FASTQ], [None], where="fq")
    check(fa, [FASTQ], [None], where="fa")
    assert mg.seq_convert_diag()["windows"] == 2 and mg.seq_convert_diag()["tiles"] == 2 * ((len(fa) + 4095) // 4096)


# ---- what MG_SEQ_HOCO carries ----

def test_hoco_carry():
    wrap = lambda s, w: b"".join(s[i:i + w] + b"\n" for i in range(0, len(s), w))
    poly = b">polyA\n" + wrap(b"A" * 10000, 60)
    for kb in WINDOWS:
        assert run_text(poly, HOCO, kb)[0] == b">polyA\nA\n"
    check(poly, [HOCO, FASTQ], where="poly-A")
    for at in (4096, 4097):                                # the run broken exactly there: byte `at` - 1 is the first C
        s = bytearray(b">r\n" + b"A" * 9000 + b"\n")
        s[at - 1:at + 99] = b"C" * 100
        check(bytes(s), [HOCO], where=("run broken", at))
    check(b">gap\nAAAA" + b" " * 5000 + b"AAAC\n" + b" " * 5000 + b"\nCCG\n", [HOCO, FASTA], where="a run around 5000 dropped bytes")
    for pre in (4092, 4093):                               # "Aa" around the window edge (byte 4096 is the next window's first)
        check(b">r\n" + b"C" * (pre - 1) + b"Aa" + b"G\n>s\nT\n", [HOCO], where=("Aa", pre))
    # the last base of a record equals the first base of the next, the '>' line on the edge: both are kept
    for pre in (4090, 4091, 4092, 4093):
        data = b">r\n" + b"CA" * ((pre - 2) // 2) + b"T\n>s\nTTG\n"
        check(data, [HOCO], where=("equal bases across a start", pre, data.index(b"\n>s")))
    # an empty record in the second window: nothing after it is written
    stop = b">a\n" + wrap(b"ACGT" * 1100, 80) + b">b\nAC\n>e\n\n>f\nACGT\n"
    assert stop.index(b">e") > 4096
    check(stop, [HOCO], where="stop in the second window")
    for kb in WINDOWS:
        assert run_text(stop, HOCO, kb)[0].endswith(b">b\nAC\n") and run_text(stop, HOCO, kb)[2]["nSeqIn"] == 2
    fq = b"".join(b"@q%d\n" % i + b"AAcCCg" * 150 + b"TTtn\n+\n" + b"I" * 904 + b"\n" for i in range(12))
    check(fq, [HOCO], where="fastq runs")


# ---- FASTA -> FASTQ: the '!' lines ----

def test_fasta_to_fastq_fill():
    rng = np.random.default_rng(33)
    one = b">one\n" + b"".join(seq(rng, 100, b"ACGT") + b"\n" for _ in range(200)) + b">two\nAC\n"
    check(one, [FASTQ], where="a '!' run across five windows")
    for kb in WINDOWS:
        out = run_text(one, FASTQ, kb)[0]
        assert out.count(b"!") == 20002 and out.endswith(b"@two\nAC\n+\n!!\n")
    check(b"".join(b">r%d\n%c\n" % (i, b"ACGT"[i % 4]) for i in range(300)), [FASTQ], where="300 records of one base")
    check(b">a\nAC\n>empty\n>b\n\n>c\nA\n", [FASTQ], where="empty records")
    check(b">only\n" + b"ACGT" * 3000 + b"\n", [FASTQ], where="one record, ended by the text's end")


def test_records_without_a_sequence_line_grow():
    """`>a\\n` is written as `>a\\n\\n`: windows of such records give up to half as many bytes again (FASTA out), three times as many (FASTQ out)"""
    for data, where in ((b"".join(b">r%d\n" % i for i in range(900)), "900 headers"), (b">\n" * 3000, "3000 bare markers"), (b">x y\n\n" * 700, "700 headers and a blank line"),
                        (b">a\nAC\n" + b">e\n" * 2500 + b">z\nACGT\n", "a run of 2500 between two records")):
        assert len(data) > 4096
        check(data, where=where)
    for kb in WINDOWS:
        out, err, res = run_text(b">\n" * 3000, FASTA, kb)
        assert len(out) == 3 * 2999 and res["nSeq"] == 2999 and res["totSeqLen"] == 0      # (the last one is a file that ends in a header line)
        assert len(run_text(b">\n" * 3000, FASTQ, kb)[0]) == 6 * 2999


# ---- random files ----

def random_file(rng, fastq):
    n_rec = int(rng.integers(1, 9))
    lens = [int(rng.choice([0, 1, int(rng.integers(0, 40)), int(rng.integers(0, 6001))])) for _ in range(n_rec)]
    parts = []
    for i, n in enumerate(lens):
        name = b"r%d" % i + ([b" ", b"\t", b"  "][int(rng.integers(0, 3))] + b"d" * int(rng.integers(0, 60)) if rng.random() < 0.5 else b"")
        if fastq:
            s = seq(rng, n, b"ACGTNacgtn.*" if rng.random() < 0.3 else b"AACCGTNacgtn")
            q = seq(rng, n, b"!\"#5II~~~~~~@+")
            parts.append(b"@" + name + b"\n" + s + b"\n+" + (name if rng.random() < 0.3 else b"") + b"\n" + q + b"\n")
        else:
            s = seq(rng, n, b"AACCGTNacgtnRYKMSWBDHV- x>@")
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
    """seeded shapes, both formats, lengths 0 to 6000, lines of random width, some cut off: the three modes, both windows, refusals included"""
    rng = np.random.default_rng(3000 + seed)
    check(random_file(rng, fastq=bool(seed & 1)), where=("seed", seed))


# ---- gzip, and the names ----

@pytest.mark.parametrize("name", ["conv_long.fa", "conv_many.fq"])
def test_gzip_in_and_out(name, tmp_path):
    data = open(os.path.join(ts.GOLDEN, name), "rb").read()
    gz = str(tmp_path / (name + ".gz"))
    open(gz, "wb").write(gzip.compress(data[:3000]) + gzip.compress(data[3000:]))      # two members: gzread reads them as one stream
    for kb in WINDOWS:
        with mg.knobs(TEXT_WINDOW_KB=kb):
            for flags, suffix in ((0, ".fa.gz"), (0, ".fq.gz"), (0, ".fq"), (HOCO, ".x.gz"), (FASTQ, ".fa")):      # the flag comes before the name
                dst = str(tmp_path / ("out%s" % suffix))
                err, res = mg.seq_convert_file(gz, dst, flags)
                want = ts.restate(data, flags or (FASTA if ".fa" in suffix else FASTQ))
                got = open(dst, "rb").read()
                assert (gzip.decompress(got) if dst.endswith(".gz") else got, err, res) == want, (name, kb, suffix)
                assert (got[:2] == b"\x1f\x8b") == dst.endswith(".gz")
    cut = str(tmp_path / (name + ".cut.gz"))               # an unfinished last record in a stream
    open(cut, "wb").write(gzip.compress(data[:-7]))
    dst = str(tmp_path / "cut.fa")
    err, res = mg.seq_convert_file(cut, dst, 0)
    assert (open(dst, "rb").read(), err, res) == ts.restate(data[:-7], FASTA) and err.startswith("incomplete sequence record line ")


def test_names_and_flags(tmp_path):
    src = os.path.join(ts.GOLDEN, "conv_mixed.fa")
    for dst, flags, match in (("out.txt", 0, "no output type"), ("out.gz", 0, "no output type"), ("out.bin.gz", 0, "no output type"), ("out.fa", 3, "at once"),
                              ("out.fq", HOCO | FASTQ, "MG_SEQ_HOCO"), ("out.fa", 8, "unknown flags"), ("-", 0, "no output type")):
        with pytest.raises(mg.ModgpuError, match=match):
            mg.seq_convert_file(src, str(tmp_path / dst) if dst != "-" else dst, flags)
        assert not os.path.exists(str(tmp_path / dst))
    for flags, match in ((0, "no output type"), (3, "at once"), (6, "MG_SEQ_HOCO"), (16, "unknown flags")):
        with pytest.raises(mg.ModgpuError, match=match):
            mg.seq_convert_text(b">a\nA\n", flags)
    for p in (str(tmp_path / "missing.fa"),):
        with pytest.raises(mg.ModgpuError, match="failed to open"):
            mg.seq_convert_file(p, str(tmp_path / "o.fa"), 0)
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    with pytest.raises(mg.ModgpuError, match="empty"):
        mg.seq_convert_file(str(empty), str(tmp_path / "o.fa"), 0)
    assert not os.path.exists(str(tmp_path / "o.fa"))
    r = subprocess.run([sys.executable, "-c", "import modimizer_amd as mg; mg.seq_convert_file(%r, '-', mg.SEQ_FASTA)" % src], capture_output=True,
                       env=dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(mg.__file__)))))
    assert r.returncode == 0 and r.stdout == ts.restate(open(src, "rb").read(), FASTA)[0], r.stderr[-400:]


# ---- refusals ----

@pytest.mark.parametrize("kb", WINDOWS)
def test_refusals(kb, tmp_path):
    good = b"@g\nACGT\n+\nIIII\n"
    pad = b"".join(b"@p%d\n" % i + b"ACGT" * 30 + b"\n+\n" + b"5" * 120 + b"\n" for i in range(40))      # the breach lies past the first tile
    n_pad, off = 160, len(pad)

    def refused(data, flags, words):
        with pytest.raises(mg.ModgpuError) as e:
            run_text(data, flags, kb)
        assert words in str(e.value) and e.value.out == b"", (str(e.value), words)
        src, dst = str(tmp_path / "in"), str(tmp_path / "out.fa")
        open(src, "wb").write(data)
        open(dst, "wb").write(b"what an earlier call left")
        with mg.knobs(TEXT_WINDOW_KB=kb):
            with pytest.raises(mg.ModgpuError) as e:
                mg.seq_convert_file(src, dst, flags)
        assert words in str(e.value) and not os.path.exists(dst)

    for flags in ALL:
        refused(pad + b"@a\nACGT\nIIII\n+\n", flags, "missing + FASTQ line %d" % (n_pad + 3))
        refused(pad + b"@a\nACGT\n\nIIII\n", flags, "missing + FASTQ line %d" % (n_pad + 3))
        refused(pad + b"@a\nACGT\n+\nIII\n" + good, flags, "qual not same length as seq line %d" % (n_pad + 4))
        refused(pad + b"@a\nACG\n+\nIIII\n" + b"@b\nACGT\n+\nIII\n", flags, "qual not same length as seq line %d" % (n_pad + 4))      # the sums agree again later: the first one counts
        refused(pad + b"a\nACGT\n+\nIIII\n", flags, "no initial @ for FASTQ record line %d" % (n_pad + 1))
        refused(pad + b"@a\nACGT\nX", flags, "missing + FASTQ line %d" % (n_pad + 3))                  # dies before the file runs out
        # a byte from 0x80 in a FASTA sequence line; in a header it is no base, in a record that is dropped it is never converted
        fa = b">h\xe9\n" + b"ACGT" * 1200 + b"\nAC\xe9T\n>b\nACGT\n"
        refused(fa, flags, "offset %d " % fa.index(b"\xe9T"))
        assert run_text(fa.replace(b"AC\xe9T", b"ACGT"), flags, kb)[2]["totSeqLenIn"] == 4808
        assert run_text(b">a\nACGT\n>b\nAC\xe9", flags, kb)[1] == "incomplete sequence record line 4\n"
        # a NUL byte in a header line, in the id and in the description
        refused(pad + b"@a\x00b\nACGT\n+\nIIII\n", flags, "offset %d " % (off + 2))
        fa = b">a\n" + b"ACGT" * 1200 + b"\n>b some\x00thing\nACGT\n"
        refused(fa, flags, "offset %d " % fa.index(b"\x00"))
    # MG_SEQ_HOCO with FASTQ in: a sequence byte outside ACGTNacgtn; the other two modes write it as it is
    fq = pad + b"@a\nAC.T\n+\nII I\n" + good
    refused(fq, HOCO, "offset %d " % (off + 5))
    assert run_text(fq, FASTA, kb)[2]["nSeq"] == 42 and run_text(fq, FASTQ, kb)[0] == fq
    refused(fq + b"@z\nAC\nII\n", HOCO, "offset %d " % (off + 5))                   # the byte's record comes before the broken rule's
    refused(pad + b"@z\nAC\n+\nI\n" + fq[off:], HOCO, "qual not same length")        # ... and the other way round
    assert run_text(good + b"@a\nAC.T\n+\nII", HOCO, kb)[2]["nSeq"] == 1             # in a record that is dropped
    assert run_text(good + b"@e\n\n+\n\n@a\nAC.T\n+\nII I\n", HOCO, kb)[0] == b">g\nACGT\n"      # behind seqhoco's stop it is never read
    for flags in ALL:
        with pytest.raises(mg.ModgpuError, match="neither FASTA nor FASTQ"):
            run_text(b"ACGT\n", flags, kb)
        with pytest.raises(mg.ModgpuError, match="empty"):
            run_text(b"", flags, kb)


# ---- the example ----

def test_example_reproduces_a_golden_of_each_mode(tmp_path):
    exe = ts.example_binary(tmp_path)
    g = {stem: (path, runs) for stem, path, runs in ts.goldens()}
    for stem, mode in (("conv_mixed_fa", "fq"), ("conv_reads_fq", "fa"), ("conv_hoco_fa", "hoco"), ("conv_cut_seq_fq", "fq")):
        path, runs = g[stem]
        want_out, want_err = ts.expected_of(stem, mode, runs[mode])
        dst = str(tmp_path / (stem + "." + mode))
        r = subprocess.run([exe, "-" + mode, dst, path], capture_output=True)
        assert (r.returncode, open(dst, "rb").read(), r.stderr.decode("latin-1")) == (0, want_out, want_err), (stem, mode)
