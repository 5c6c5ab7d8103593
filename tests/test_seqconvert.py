"""`seqconvert -fa|-fq` (seqconvert.c) and `seqhoco` (seqhoco.c) over seqIOread / seqIOwrite (seqio.c:234-346,463-545): a plain restatement
of the rules include/modgpu.h states for mgSeqConvertFile, record by record as the programs read them, against the programs' own output
(tests/golden/conv_*: make_golden_seqconvert.py), which the GPU tests (test_gpu_seqconvert.py) then lean on; the names in header, library
and binding; the example compiles.

seqhoco appends one byte from beyond the sequence to every sequence line (seqhoco.c:29-30): the goldens must show it, and with it removed
the line is the restatement's."""
import glob
import json
import os
import re
import subprocess

import pytest

import modimizer_amd as mg
from tests import util

GOLDEN = os.path.join(util.ROOT, "tests", "golden")
FASTA, FASTQ, HOCO = 1, 2, 4
MODES = {"fa": FASTA, "fq": FASTQ, "hoco": HOCO}
NAMES = {"mgSeqConvertFile": "int  ", "mgSeqConvertText": "int  ", "mgSeqConvertDiag": "void "}
AMBIG = {ord(c): ord(c.upper()) for c in "ABCDGHKMNRSTVWYabcdghkmnrstvwy"}      # dna2textAmbigConv, seqio.c:621-630
AMBIG[ord("-")] = ord("-")
ACGTN = set(b"ACGTNacgtn")                                                         # dna2textConv
SPACE = set(b" \t\n\v\f\r")                                                        # isspace in the C locale
MAXLEN = 1 << 31


class Refused(Exception):
    """.kind: 'rule' (args[0] = the program's words), 'byte' (.offset), 'long', 'open', 'flags'"""
    def __init__(self, kind, msg, offset=None):
        Exception.__init__(self, msg)
        self.kind, self.offset = kind, offset


def read_records(data):
    """generator of (header start, header line less marker and newline, seq offset, seq bytes as in the file, qual bytes or None), then
    one ('end', stderr text).  Raises Refused ('rule') where the reader die()s"""
    n = len(data)
    fastq = data[0] == ord("@")
    line, pos = 1, 0

    def line_end(p, in_record_newline):
        """the newline that ends the line p is in; None where the reader runs out of bytes inside the record (bufAdvanceInRecord,
        seqio.c:215-219): no newline, or -- for the lines whose newline is stepped over inside the record -- a newline that is the last byte"""
        e = data.find(b"\n", p)
        if e < 0:
            return None, line
        if in_record_newline and e == n - 1:
            return None, line + 1
        return e, line

    def incomplete(at):
        return ("end", "incomplete sequence record line %d\n" % at)

    while pos < n:
        start = pos
        if fastq and data[pos] != ord("@"):
            raise Refused("rule", "no initial @ for FASTQ record line %d" % line)
        e, at = line_end(pos, True)
        if e is None:
            yield incomplete(at)
            return
        header = data[pos + 1:e]
        line += 1
        pos = e + 1
        if not fastq:
            seq_at = pos
            while pos < n and data[pos] != ord(">"):
                e, at = line_end(pos, False)
                if e is None:
                    yield incomplete(at)
                    return
                line += 1
                pos = e + 1
            yield (start, header, seq_at, data[seq_at:pos], None)
            continue
        e, at = line_end(pos, True)
        if e is None:
            yield incomplete(at)
            return
        seq_at, seq = pos, data[pos:e]
        line += 1
        pos = e + 1
        if data[pos] != ord("+"):
            raise Refused("rule", "missing + FASTQ line %d" % line)
        e, at = line_end(pos, True)
        if e is None:
            yield incomplete(at)
            return
        line += 1
        pos = e + 1
        e, at = line_end(pos, False)
        if e is None:
            yield incomplete(at)
            return
        if e - pos != len(seq):
            raise Refused("rule", "qual not same length as seq line %d" % line)
        yield (start, header, seq_at, seq, data[pos:e])
        line += 1
        pos = e + 1
    yield ("end", "")


def split_header(header):
    """(id, description): seqio.c:303-313"""
    i = 0
    while i < len(header) and header[i] not in SPACE:
        i += 1
    return header[:i], header[i + 1:]


def hoco(seq):
    out = bytearray()
    for c in seq:
        if not out or (c & 0xdf) != (out[-1] & 0xdf):      # toupper of a letter of ACGTNacgtn
            out.append(c)
    return bytes(out)


def restate(data, flags):
    """(output bytes, stderr text, result dict) of the conversion `flags` ask for on the bytes `data`; raises Refused"""
    data = bytes(data)
    if flags & ~7 or (flags & FASTA and flags & FASTQ) or (flags & HOCO and flags & FASTQ) or not flags:
        raise Refused("flags", "flags")
    if not data:
        raise Refused("open", "unreadable or empty")
    if data[0] not in b">@":
        raise Refused("open", "neither FASTA nor FASTQ")
    fastq_in, fastq_out, is_hoco = data[0] == ord("@"), bool(flags & FASTQ), bool(flags & HOCO)
    out, err = [], ""
    r = dict(inType=2 if fastq_in else 1, outType=2 if fastq_out else 1, nSeq=0, totSeqLen=0, maxSeqLen=0, totIdLen=0, totDescLen=0, maxIdLen=0, maxDescLen=0,
             nSeqIn=0, totSeqLenIn=0)
    for rec in read_records(data):
        if rec[0] == "end":
            err = rec[1]
            break
        start, header, seq_at, seq, qual = rec
        if 0 in header:
            raise Refused("byte", "a NUL byte in a header line", start + 1 + header.index(0))
        ident, desc = split_header(header)
        if is_hoco:
            desc = b""
        if not fastq_in:
            hi = [i for i, c in enumerate(seq) if c >= 0x80]
            if hi:
                raise Refused("byte", "convert[] out of bounds", seq_at + hi[0])
            seq = bytes(c for c in seq if c in ACGTN) if is_hoco else bytes(AMBIG[c] for c in seq if c in AMBIG)
        elif is_hoco:
            bad = [i for i, c in enumerate(seq) if c not in ACGTN]
            if bad:
                raise Refused("byte", "convert[] out of bounds", seq_at + bad[0])
        if len(seq) >= MAXLEN:
            raise Refused("long", "a record of 2^31 bases or more")
        if is_hoco and not seq:
            break                                           # seqhoco.c:26
        r["nSeqIn"] += 1
        r["totSeqLenIn"] += len(seq)
        if is_hoco:
            seq = hoco(seq)
        r["nSeq"] += 1
        r["totSeqLen"] += len(seq)
        r["maxSeqLen"] = max(r["maxSeqLen"], len(seq))
        r["totIdLen"] += len(ident)
        r["maxIdLen"] = max(r["maxIdLen"], len(ident))
        r["totDescLen"] += len(desc)
        r["maxDescLen"] = max(r["maxDescLen"], len(desc))
        out.append((b"@" if fastq_out else b">") + ident + (b" " + desc if desc else b"") + b"\n" + seq + b"\n")
        if fastq_out:
            out.append(b"+\n" + (qual if qual is not None else b"!" * len(seq)) + b"\n")
    return b"".join(out), err, r


# ---- the goldens ----

def goldens():
    """[(json file's stem, input path, {mode: run})]"""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "conv_*.json"))):
        g = json.load(open(p))
        out.append((os.path.basename(p)[:-5], os.path.join(GOLDEN, g["input"]), g["runs"]))
    return out


def strip_hoco_junk(stem, program_out):
    """seqhoco's stdout less the one byte it appends to every sequence line -- which must be there, and be no base"""
    lines = program_out.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1, stem
    for i in range(1, len(lines) - 1, 2):
        assert lines[i] and lines[i][-1] not in ACGTN and all(c in ACGTN for c in lines[i][:-1]), (stem, i, lines[i][-8:])
        lines[i] = lines[i][:-1]
    return b"\n".join(lines)


def expected_of(stem, mode, run):
    """what the device must write for a recorded run: (stdout, stderr) or the program's last words"""
    if run["status"]:
        assert run["status"] == 255 and run["stderr"].startswith("FATAL ERROR: ")
        return None, run["stderr"][len("FATAL ERROR: "):].strip()
    out = run["stdout"].encode("latin-1")
    return (strip_hoco_junk(stem, out) if mode == "hoco" else out), run["stderr"]


def test_goldens_are_there():
    names = {g[0] for g in goldens()}
    assert {"conv_headers_fa", "conv_headers_fq", "conv_mixed_fa", "conv_empty_mid_fa", "conv_empty_end_fa", "conv_long_fa", "conv_hoco_fa", "conv_hoco_stop_fa",
            "conv_reads_fq", "conv_many_fq", "conv_odd_fq", "conv_crlf_fq", "conv_nonl_fa", "conv_hdr_end_fa", "conv_hdr_only_fa", "conv_hdr_nonl_fa",
            "conv_cut_seq_fq", "conv_cut_qual_fq", "conv_cut_hdr_fq", "conv_cut_only_fq", "conv_die_plus_fq", "conv_die_qual_fq", "conv_die_at_fq"} <= names
    for stem, path, runs in goldens():
        assert {"fa", "fq"} <= set(runs) <= set(MODES), stem
        assert os.path.getsize(path) < 100000


@pytest.mark.parametrize("stem,path,runs", goldens(), ids=[g[0] for g in goldens()])
def test_restatement_vs_reference_programs(stem, path, runs):
    """seqconvert's stdout and stderr byte for byte; seqhoco's with the byte it appends to every sequence line asserted and removed"""
    data = open(path, "rb").read()
    for mode, run in runs.items():
        want_out, want_err = expected_of(stem, mode, run)
        if want_out is None:
            with pytest.raises(Refused) as r:
                restate(data, MODES[mode])
            assert r.value.kind == "rule" and str(r.value) == want_err, (stem, mode)
            continue
        out, err, res = restate(data, MODES[mode])
        assert (out, err) == (want_out, want_err), (stem, mode)
        assert res["outType"] == (2 if mode == "fq" else 1) and res["nSeq"] == out.count(b"\n") // (4 if mode == "fq" else 2)


def test_fixtures_hold_what_they_are_for():
    g = {stem: (open(path, "rb").read(), runs) for stem, path, runs in goldens()}
    h = g["conv_headers_fa"][1]["fa"]["stdout"]
    assert ">r1 desc with\ttab\n" in h and ">r2\n" in h and ">r4  two\n" in h and "\n>\nACGTAC\n" in h and "\n> only a description\n" in h and ">r7\nACGTACG\n" in h
    assert ">r8 crlf too\r\n" in h and ">r10 a > inside\nACGT\n" in h
    assert g["conv_headers_fa"][1]["hoco"]["stdout"].startswith(">r1\nACGT")
    assert "@q1 desc with\ttab\nACGT\n+\nIIII\n" in g["conv_headers_fq"][1]["fq"]["stdout"] and "\n@\nACGT\n" in g["conv_headers_fq"][1]["fq"]["stdout"]
    assert ">b\n\n>c\n" in g["conv_empty_mid_fa"][1]["fa"]["stdout"] and "@b\n\n+\n\n@c\n" in g["conv_empty_mid_fa"][1]["fq"]["stdout"]
    assert g["conv_empty_mid_fa"][1]["hoco"]["stdout"].count(">") == 1 and g["conv_hoco_stop_fa"][1]["hoco"]["stdout"].count(">") == 2
    m = g["conv_mixed_fa"][1]["fa"]["stdout"]
    assert "\nACGTACGTNNRYKMSWBDHVRYKMSWBDHV--ACGT\n" in m and "\nACGTXXACGT\n" not in m and "+\n!!!!!!!!!!" in g["conv_mixed_fa"][1]["fq"]["stdout"]
    hc = strip_hoco_junk("conv_hoco_fa", g["conv_hoco_fa"][1]["hoco"]["stdout"].encode("latin-1"))
    assert b">h1\nACGTACGT\n>h2\nA\n>h3\na\n>h4\ncgtNA\n>h5\nACGT\n>h6\nTGCA\n" in hc and hc.endswith(b">h8\nAC\n")
    assert g["conv_reads_fq"][1]["fq"]["stdout"].count("\n+\n") >= 8 and b"\n+q1 some" in g["conv_reads_fq"][0] and b"\n\n+" in g["conv_reads_fq"][0]
    assert "AC*GT\r\n" in g["conv_odd_fq"][1]["fa"]["stdout"] and "AC\xe9T.\n" in g["conv_odd_fq"][1]["fq"]["stdout"]
    assert len(g["conv_long_fa"][0]) > 4096 + 2000 and len(g["conv_many_fq"][0]) > 4096
    for stem in ("conv_nonl_fa", "conv_hdr_end_fa", "conv_cut_seq_fq", "conv_cut_qual_fq", "conv_cut_hdr_fq"):
        assert g[stem][1]["fa"]["stderr"].startswith("incomplete sequence record line ") and g[stem][1]["fa"]["stdout"], stem


def test_restatement_refuses_what_the_programs_cannot_do():
    with pytest.raises(Refused) as r:
        restate(b">a\nAC\xe9T\n", FASTA)
    assert r.value.kind == "byte" and r.value.offset == 5
    assert restate(b">a\xe9\nACT\n", FASTA)[0] == b">a\xe9\nACT\n"          # in a header it is no base
    assert restate(b">a\nACT\n>b\nAC\xe9", FASTA)[0] == b">a\nACT\n"          # in the unfinished record it is never converted
    with pytest.raises(Refused) as r:
        restate(b">a\nACT\n>b\x00c\nAC\n", FASTQ)
    assert r.value.kind == "byte" and r.value.offset == 9
    fq = b"@a\nACxT\n+\nIIII\n"
    assert restate(fq, FASTA)[0] == b">a\nACxT\n" and restate(fq, FASTQ)[0] == fq
    with pytest.raises(Refused) as r:
        restate(fq, HOCO)
    assert r.value.kind == "byte" and r.value.offset == 5
    assert restate(b">a\nAC\n>e\n\n>b\nA\xe9\n", HOCO)[0] == b">a\nAC\n"       # seqhoco never reads past the empty record
    for bad in (b"", b"ACGT\n", b"b123"):
        with pytest.raises(Refused) as r:
            restate(bad, FASTA)
        assert r.value.kind == "open"
    for flags in (0, 3, 6, 7, 8):
        with pytest.raises(Refused) as r:
            restate(b">a\nA\n", flags)
        assert r.value.kind == "flags"
    assert restate(b">x  y\naAaA\nAc\n", HOCO) == (b">x\nac\n", "", dict(inType=1, outType=1, nSeq=1, totSeqLen=2, maxSeqLen=2, totIdLen=1, totDescLen=0, maxIdLen=1,
                                                                      maxDescLen=0, nSeqIn=1, totSeqLenIn=6))
    assert restate(b">x  y\naa\n", FASTQ)[0] == b"@x  y\nAA\n+\n!!\n" and restate(b">x  y\naa\n", FASTQ)[2]["maxDescLen"] == 2


# ---- names, example ----

def test_names_in_header_library_and_binding():
    header = open(os.path.join(util.ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n, ret in NAMES.items():
        assert re.search(r"^%s%s \(" % (re.escape(ret), n), header, re.M), n
        assert n in mg.EXPORTS and hasattr(L, n), n
    assert "} MgSeqConvert ;" in header and all(re.search(r"^#define MG_SEQ_%s %d$" % (k, v), header, re.M) for k, v in (("FASTA", 1), ("FASTQ", 2), ("HOCO", 4)))
    assert (mg.SEQ_FASTA, mg.SEQ_FASTQ, mg.SEQ_HOCO) == (FASTA, FASTQ, HOCO)
    assert callable(mg.seq_convert_file) and callable(mg.seq_convert_text) and callable(mg.seq_convert_diag)
    assert "mg_seqconvert.o" in open(os.path.join(mg.CSRC, "Makefile")).read() and os.path.exists(os.path.join(mg.CSRC, "mg_seqconvert.hip"))


def test_no_device_no_conversion(tmp_path):
    """like every batch entry point: without a HIP device the call fails and says so; there is no host conversion"""
    if mg.lib().mgDeviceCount() > 0:
        return
    out = str(tmp_path / "o.fa")
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.seq_convert_file(os.path.join(GOLDEN, "conv_mixed.fa"), out, FASTA)
    assert not os.path.exists(out)
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.seq_convert_text(b">a\nACGT\n", FASTA)


def example_binary(tmp_path):
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    mg.lib()
    exe = str(tmp_path / "convert_file")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "convert_file.c"),
                        "-o", exe, "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_example_compiles(tmp_path):
    example_binary(tmp_path)
