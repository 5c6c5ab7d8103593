#!/usr/bin/env python3
"""Generate tests/golden/conv_* by running the REFERENCE ITSELF: its seqconvert.c and seqhoco.c are compiled here into a temporary
directory (oracle/ does not build them), with the line make_golden_composition.py uses, run on the inputs this script writes, and deleted
with the directory.  Only where the reference's sources are.  The outputs are data: inputs and the programs' answers.  Re-run with:
    python tests/golden/make_golden_seqconvert.py

  conv_<name>.fa / .fq     an input
  conv_<name>_<fa|fq>.json {"input": file name, "what": one line, "runs": {"fa" | "fq" | "hoco": {"stdout", "stderr", "status"}}}:
                           `seqconvert -fa -S input`, `seqconvert -fq -S input` (stdout as written) and `seqhoco input` (stdout gunzipped;
                           "" where gzip found nothing to inflate)

-S always: without it the program's closing report crashed here when it wrote to a named file.  seqhoco appends one byte from beyond the
sequence to every sequence line it writes (seqhoco.c:29-30 reads seq[seqLen]); the inputs' sequence lines all end in a newline, where that
byte was 0xFE in every run here.  "hoco" is not recorded for inputs on which seqhoco would index a table out of bounds (FASTQ with other
bytes than ACGTNacgtn in a sequence line) or whose unfinished last record has bases on its last line."""
import gzip
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MODGPU_REFERENCE_SRC", "/root/reference")
assert os.path.exists(os.path.join(REF, "seqconvert.c")), "needs the reference's sources"

ALL = ("fa", "fq", "hoco")
NOHOCO = ("fa", "fq")


def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width)) if len(seq) else b""


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).tobytes())


def fasta(recs, width=60):
    return b"".join(b">" + name + b"\n" + wrap(seq, width) for name, seq in recs)


def fastq(recs, plus=b"+"):
    return b"".join(b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n" for name, seq, qual in recs)


def quals(rng, n):
    return bytes(rng.integers(33, 127, n, dtype=np.uint8).tobytes())


def inputs():
    rng = np.random.default_rng(20201208)
    out = {}
    # the header shapes: tab separator, trailing space, double space, empty id, CRLF
    hdr = (b">r1\tdesc with\ttab\nACGT\n>r2 \nACGTA\n>r3\nAC\n>r4  two\nACG\n>\nACGTAC\n> only a description\nA\n>r7\r\nACGTACG\n"
           b">r8 crlf too\r\nAC\n>r9\x0bvt\x0cff\nACGTT\n>r10 a > inside\nAC>GT\n")
    out["headers.fa"] = ("header shapes: tab, trailing space, double space, empty id, CRLF", hdr, ALL)
    hq = b"".join(b"@" + h + b"\nACGT\n+\nIIII\n" for h in (b"q1\tdesc with\ttab", b"q2 ", b"q3", b"q4  two", b"", b" only a description", b"q7\r", b"q8 x\r"))
    out["headers.fq"] = ("the same in FASTQ", hq, ALL)
    mixed = (b">r1 mixed case and ambiguity codes > not a start\nACGTacgtNnRYKMSWBDHV\nrykmswbdhv--ACGT\n\n"
             b">r2\tdropped bytes\nAC GT*12xX.EFIJLOPQUZ\nefijlopquz\tACGT\r\n>r3\n" + wrap(rand_seq(rng, 1200, b"ACGTN"), 70)
             + b">r4\n" + wrap(rand_seq(rng, 431), 61) + b"\n\n>r5\nA\n>r6\n" + wrap(rand_seq(rng, 477, b"acgtRY-"), 50))
    out["mixed.fa"] = ("mixed case, ambiguity codes, '-', dropped bytes, blank lines, multi-line records", mixed, ALL)
    out["empty_mid.fa"] = ("lengths 5, 0, 100: an empty record is written with empty lines; seqhoco stops at it", b">a\nACGTA\n>b\n>c\n" + wrap(rand_seq(rng, 100), 60), ALL)
    out["empty_end.fa"] = ("a trailing empty record", b">a\nACGTACG\n>b\n" + wrap(rand_seq(rng, 150), 60) + b">c\n\n", ALL)
    lens = [1, 6000, int(rng.integers(200, 400)), 0, 17]
    out["long.fa"] = ("records of 0 to 6000 bases, the longest over two tiles", fasta([(b"L%d len=%d" % (i, n), rand_seq(rng, n, b"ACGTacgtN")) for i, n in enumerate(lens)], 77), ALL)
    # homopolymers: runs over line breaks, one of several lines, aAaA, equal bases either side of a record start
    hoco = (b">h1 runs cross the line breaks\nACGGGTTTA\nAAACCCCCG\nGGT\n>h2 several lines of one base\n" + wrap(b"A" * 250, 60) + b">h3\naAaA\n>h4\nccCCgGtT\nTtNnnA\n"
            b">h5 ends in T\nACGT\n>h6 starts with T\nTTGCA\n>h7\n" + wrap(rand_seq(rng, 600, b"AACCGGTTacgtN"), 64) + b">h8 dropped bytes inside a run\nAA AA\nA-A*AxA\nC\n")
    out["hoco.fa"] = ("homopolymer runs: over line breaks, several lines, aAaA, equal bases across a record start, dropped bytes inside a run", hoco, ALL)
    out["hoco_stop.fa"] = ("an empty record in the middle: seqhoco stops there", b">a\nAACCGGTT\n>b\nACGT\n>empty\n\n>d\nAAAA\n>e\nAC\n", ALL)
    # FASTQ: '+id' lines, an empty record, '@' and '+' as first quality bytes
    recs = []
    for i, n in enumerate([150, 0, 151, 37, 150, 1200, 5, 149]):
        q = bytearray(quals(rng, n))
        if n >= 2:
            q[0] = b"@+"[i % 2]
        recs.append((b"q%d some description" % i, rand_seq(rng, n, b"ACGTNacgt"), bytes(q)))
    fq = b"".join(b"@" + nm + b"\n" + s + b"\n+" + (nm if i % 2 else b"") + b"\n" + q + b"\n" for i, (nm, s, q) in enumerate(recs))
    out["reads.fq"] = ("'+id' lines, an empty record, '@' and '+' as first quality bytes, records of 0 to 1200 bases", fq, ALL)
    many = [(b"m%d" % i, rand_seq(rng, n, b"AACCGGTTacgtN"), quals(rng, n)) for i, n in enumerate(int(x) for x in rng.integers(1, 400, 12))]
    out["many.fq"] = ("twelve records over more than one tile, none empty", fastq(many), ALL)
    odd = b"@o1\nAC*GT\r\n+\nIIIII!\n@o2 x\nAC\xe9T.\n+o2\n~~~~~\n"
    out["odd.fq"] = ("'*', '\\r' and a byte >= 0x80 in sequence lines: written as they are", odd, NOHOCO)
    crlf = b"".join(b"@c%d\r\n" % i + s + b"\r\n+\r\n" + b"I" * len(s) + b"\r\n" for i, s in enumerate([rand_seq(rng, 40), rand_seq(rng, 75)]))
    out["crlf.fq"] = ("CRLF line ends", crlf, NOHOCO)
    # a last record the programs drop as unfinished
    two = b">a\n" + wrap(rand_seq(rng, 90), 50) + b">b\n" + wrap(rand_seq(rng, 333), 50)
    out["nonl.fa"] = ("no final newline: the last record is dropped", two + b">c\nACGTACGTAC", NOHOCO)
    out["hdr_end.fa"] = ("the file ends in a header line", two + b">c and nothing else\n", ALL)
    out["hdr_only.fa"] = ("one header line: nothing is written", b">alone\n", ALL)
    out["hdr_nonl.fa"] = ("one header line without its newline", b">alone", ALL)
    good = fastq([(b"g%d" % i, s, b"5" * len(s)) for i, s in enumerate([rand_seq(rng, 100), rand_seq(rng, 52), rand_seq(rng, 77)])])
    out["cut_seq.fq"] = ("ends after a record's sequence line", good + b"@cut\nACGTACGT\n", ALL)
    out["cut_qual.fq"] = ("ends inside a quality line", good + b"@cut\nACGTACGT\n+\n5555", ALL)
    out["cut_hdr.fq"] = ("ends inside a header line", good + b"@cu", ALL)
    out["cut_only.fq"] = ("one unfinished record", b"@cut\nACGT\n+\n", ALL)
    # FASTQ that breaks a rule: the programs die
    out["die_plus.fq"] = ("line 7 does not start with '+'", good[:good.index(b"@g1")] + b"@g1\nACGT\nACGT\n5555\n", ALL)
    out["die_qual.fq"] = ("the second record's quality line is one byte short", good[:good.index(b"@g1")] + b"@g1\nACGTA\n+\n5555\n" + good[good.index(b"@g2"):], ALL)
    out["die_at.fq"] = ("the second record does not start with '@'", good[:good.index(b"@g1")] + b"g1\nACGT\n+\n5555\n", ALL)
    return out


def gunzip(b):
    try:
        return gzip.decompress(b) if b else b""
    except (OSError, EOFError):
        return b""


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="seqconvert_golden_")
    try:
        lib_src = [os.path.join(REF, f) for f in ("seqio.c", "utils.c", "array.c", "hash.c", "dict.c")]
        progs = {}
        for p in ("seqconvert", "seqhoco"):
            progs[p] = os.path.join(tmp, p + "_ref")
            subprocess.check_call(["gcc", "-O2", "-w", "-no-pie", "-o", progs[p], os.path.join(REF, p + ".c")] + lib_src + ["-lz", "-l:libbsd.so.0", "-lm"])
        for name, (what, data, modes) in sorted(inputs().items()):
            path = os.path.join(HERE, "conv_" + name)
            open(path, "wb").write(data)
            runs = {}
            for m in modes:
                if m == "hoco":
                    r = subprocess.run([progs["seqhoco"], "conv_" + name], capture_output=True, cwd=HERE)
                    stdout = gunzip(r.stdout)
                else:
                    r = subprocess.run([progs["seqconvert"], "-" + m, "-S", "conv_" + name], capture_output=True, cwd=HERE)
                    stdout = r.stdout
                runs[m] = {"stdout": stdout.decode("latin-1"), "stderr": r.stderr.decode("latin-1"), "status": r.returncode}
            json.dump({"input": "conv_" + name, "what": what, "runs": runs}, open(os.path.join(HERE, "conv_" + name.rsplit(".", 1)[0] + "_" + name.rsplit(".", 1)[1] + ".json"), "w"), indent=1)
            print("conv_" + name, len(data), "bytes;", {m: (v["status"], len(v["stdout"]), v["stderr"].strip()[:60]) for m, v in runs.items()})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
