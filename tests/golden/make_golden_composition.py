#!/usr/bin/env python3
"""Generate tests/golden/comp_* by running the REFERENCE ITSELF: its composition.c is compiled here into a temporary directory (oracle/
does not build it), with the line make_golden_modrep.py uses for modrep, run on the inputs this script writes, and deleted with the
directory.  Only where the reference's sources are.  The outputs are data: inputs and the program's answers.  Re-run with:
    python tests/golden/make_golden_composition.py

  comp_<name>.fa / .fq     an input
  comp_<name>_<fa|fq>.json {"input": file name, "what": one line, "runs": {flags: {"stdout", "stderr", "status"}}}, flags a subset of
                           "bql" in that order ("" = no flag): `composition [-b] [-q] [-l] input`

Every input is run under all eight subsets but comp_crlf.fq, whose quality lines hold a '\\r': with -q the program indexes totQual[13 - 33]
(composition.c:71), so only the four subsets without q are recorded.  The comp_die_* inputs break a FASTQ rule: the program die()s
(status 255) before it prints anything."""
import itertools
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MODGPU_REFERENCE_SRC", "/root/reference")
assert os.path.exists(os.path.join(REF, "composition.c")), "needs the reference's sources"

SUBSETS = ["".join(c) for r in range(4) for c in itertools.combinations("bql", r)]


def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width)) if len(seq) else b""


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).tobytes())


def fasta(recs, width=60):
    return b"".join(b">" + name + b"\n" + wrap(seq, width) for name, seq in recs)


def fastq(recs, plus=b"+"):
    return b"".join(b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n" for name, seq, qual in recs)


def skewed_quals(rng, n):
    """mostly one symbol, as a HiFi read's; 33 and 126 present in a long enough line"""
    q = np.full(n, ord("~"), np.uint8)
    low = rng.random(n) < 0.08
    q[low] = rng.integers(33, 127, int(low.sum()))
    return q.tobytes()


def inputs():
    rng = np.random.default_rng(20201207)
    out = {}
    # mixed case, ambiguity codes, '-', dropped bytes, blank lines, several lines a record, a header with a description and a '>' inside
    mixed = (b">r1 mixed case and ambiguity codes > not a start\nACGTacgtNnRYKMSWBDHV\nrykmswbdhv--ACGT\n\n"
             b">r2\tdropped bytes\nAC GT*12xX.EFIJLOPQUZ\nefijlopquz\tACGT\r\n>r3\n" + wrap(rand_seq(rng, 3000, b"ACGTN"), 70)
             + b">r4\n" + wrap(rand_seq(rng, 431), 61) + b"\n\n>r5\nA\n>r6\n" + wrap(rand_seq(rng, 977, b"acgtRY-"), 50))
    out["mixed.fa"] = ("mixed case, ambiguity codes, '-', dropped bytes, blank lines, multi-line records", mixed, SUBSETS)
    out["empty_mid.fa"] = ("lengths 5, 0, 100: lenMin is 100", b">a\nACGTA\n>b\n>c\n" + wrap(rand_seq(rng, 100), 60), SUBSETS)
    out["empty_end.fa"] = ("a trailing empty record: lenMin is 0", b">a\nACGTACG\n>b\n" + wrap(rand_seq(rng, 150), 60) + b">c\n\n", SUBSETS)
    out["single.fa"] = ("one record", b">only one\n" + wrap(rand_seq(rng, 500), 80), SUBSETS)
    out["equal.fa"] = ("all records of one length: no -l section", fasta([(b"e%d" % i, rand_seq(rng, 120)) for i in range(7)]), SUBSETS)
    lens = [int(x) for x in rng.integers(0, 6001, 9)] + [0, 1, 6000]
    out["long.fa"] = ("records of 0 to 6000 bases over several tiles", fasta([(b"L%d len=%d" % (i, n), rand_seq(rng, n, b"ACGTacgtN")) for i, n in enumerate(lens)], 77), SUBSETS)
    # FASTQ: '+id' lines, an empty sequence line, qualities 33 and 126
    recs = []
    for i, n in enumerate([150, 0, 151, 37, 150, 1200, 5, 149]):
        q = bytearray(skewed_quals(rng, n))
        if n >= 2:
            q[0], q[-1] = 33, 126
        recs.append((b"q%d some description" % i, rand_seq(rng, n, b"ACGTN"), bytes(q)))
    fq = b"".join(b"@" + nm + b"\n" + s + b"\n+" + (nm if i % 2 else b"") + b"\n" + q + b"\n" for i, (nm, s, q) in enumerate(recs))
    out["reads.fq"] = ("'+id' lines, an empty sequence line, qualities 33 and 126", fq, SUBSETS)
    many = [(b"m%d" % i, rand_seq(rng, n, b"ACGTacgtN"), skewed_quals(rng, n)) for i, n in enumerate(int(x) for x in rng.integers(0, 900, 60))]
    out["many.fq"] = ("sixty records over several tiles, '@' and '+' as quality bytes at line starts", fastq([(nm, s, (b"@+"[i % 2:i % 2 + 1] + q[1:]) if len(q) else q) for i, (nm, s, q) in enumerate(many)]), SUBSETS)
    crlf = b"".join(b"@c%d\r\n" % i + s + b"\r\n+\r\n" + bytes([ord("I")]) * len(s) + b"\r\n" for i, s in enumerate([rand_seq(rng, 40), rand_seq(rng, 75), rand_seq(rng, 12)]))
    out["crlf.fq"] = ("CRLF line ends: the '\\r' of every sequence line is an unprintable base (without -q)", crlf, [s for s in SUBSETS if "q" not in s])
    # a last record the reference drops as unfinished
    two = b">a\n" + wrap(rand_seq(rng, 90), 50) + b">b\n" + wrap(rand_seq(rng, 333), 50)
    out["nonl.fa"] = ("no final newline: the last record is dropped", two + b">c\nACGTACGTAC", SUBSETS)
    out["hdr_end.fa"] = ("the file ends in a header line", two + b">c and nothing else\n", SUBSETS)
    out["hdr_only.fa"] = ("one header line: 0 sequences, the average is -nan", b">alone\n", SUBSETS)
    out["hdr_nonl.fa"] = ("one header line without its newline", b">alone", SUBSETS)
    good = fastq([(b"g%d" % i, s, b"5" * len(s)) for i, s in enumerate([rand_seq(rng, 100), rand_seq(rng, 52), rand_seq(rng, 77)])])
    out["cut_seq.fq"] = ("ends after a record's sequence line", good + b"@cut\nACGTACGT\n", SUBSETS)
    out["cut_qual.fq"] = ("ends inside a quality line (too short, and never judged)", good + b"@cut\nACGTACGT\n+\n5555", SUBSETS)
    out["cut_hdr.fq"] = ("ends inside a header line", good + b"@cu", SUBSETS)
    out["cut_only.fq"] = ("one unfinished record", b"@cut\nACGT\n+\n", SUBSETS)
    # FASTQ that breaks a rule: the program dies before it prints
    out["die_plus.fq"] = ("line 7 does not start with '+'", good[:good.index(b"@g1")] + b"@g1\nACGT\nACGT\n5555\n", SUBSETS)
    out["die_qual.fq"] = ("the second record's quality line is one byte short", good[:good.index(b"@g1")] + b"@g1\nACGTA\n+\n5555\n" + good[good.index(b"@g2"):], SUBSETS)
    out["die_at.fq"] = ("the second record does not start with '@'", good[:good.index(b"@g1")] + b"g1\nACGT\n+\n5555\n", SUBSETS)
    return out


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="composition_golden_")
    try:
        prog = os.path.join(tmp, "composition_ref")
        lib_src = [os.path.join(REF, f) for f in ("seqio.c", "utils.c", "array.c", "hash.c", "dict.c")]
        subprocess.check_call(["gcc", "-O2", "-w", "-no-pie", "-o", prog, os.path.join(REF, "composition.c")] + lib_src + ["-lz", "-l:libbsd.so.0", "-lm"])
        for name, (what, data, subsets) in sorted(inputs().items()):
            path = os.path.join(HERE, "comp_" + name)
            open(path, "wb").write(data)
            runs = {}
            for s in subsets:
                r = subprocess.run([prog] + ["-" + c for c in s] + ["comp_" + name], capture_output=True, cwd=HERE)
                runs[s] = {"stdout": r.stdout.decode("latin-1"), "stderr": r.stderr.decode("latin-1"), "status": r.returncode}
            json.dump({"input": "comp_" + name, "what": what, "runs": runs}, open(os.path.join(HERE, "comp_" + name.rsplit(".", 1)[0] + "_" + name.rsplit(".", 1)[1] + ".json"), "w"), indent=1)
            print("comp_" + name, len(data), "bytes;", sorted({v["status"] for v in runs.values()}), runs[subsets[0]]["stdout"].splitlines()[:1], runs[subsets[0]]["stderr"].strip())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
