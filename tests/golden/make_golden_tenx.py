#!/usr/bin/env python3
"""Generate tests/golden/tenx_* by running the REFERENCE ITSELF (oracle/_ref/modutils_ref, built from the reference tree by
oracle/Makefile): modutils -x, -s, -sM and the summary every command ends in (modutils.c:33-51,205-219; modset.c:130-153).
Re-run with:  python tests/golden/make_golden_tenx.py

Inputs (written here, deterministic, committed):
  tenx_reads.fq   101 records (an odd number), four lines each; N and lower case among the bases
  tenx_reads.fa   100 records in lines of 17 / 29 / 60 bases: the first line is shorter than the 23 bases an odd record loses, and holds
                  lower case and N among them
Both hold odd records of exactly 23, 24, 23 + k - 1 and 23 + k bases for both values of k below, even records shorter than k, and no
odd record of fewer than 23 bases: the reference aborts on one (assert (len >= 0), seqhash.c:156), so no golden exists for it.

Per tag of TAGS (B k w s; k11w4 has k <= 23: a barcode left in would have hashed) and per input (fq / fa), from
  modutils_ref -c B k w s -x reads -s C1 C2 CM -sM M -H his -wt dump -w mod
  tenx_<tag>_<in>.stdout.txt   what the run prints, without the timing lines
  tenx_<tag>_<in>.hist.txt     the -H file
  tenx_<tag>_<in>.dump.txt     the -wt file
  tenx_<tag>_<in>.mod          the .mod (gzip, as its fzopen writes it)
Every file stays under 150 KiB.
"""
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MU = os.path.join(ROOT, "oracle", "_ref", "modutils_ref")
TAGS = {"k11w4": (20, 11, 4, 17), "k25w3": (20, 25, 3, 17)}
COPY = (2, 3, 6)          # -s copy1min copy2min copyMmin
COPY_M = 5                # -sM copyMmin
LIMIT = 150 * 1024
GENOME = 1200
# lengths at the head of each file, record numbers from 1: odd ones at every edge of the trim for k = 11 and k = 25, even ones shorter than k
HEAD = [23, 5, 24, 10, 33, 1, 34, 24, 47, 12, 48, 9, 23, 150]


def strip_timing(text):
    return "\n".join(l for l in text.splitlines() if not l.startswith("user\t") and "resources used" not in l
                     and not l.startswith("total resources")) + "\n"


def reads(rng, genome, n):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    out = []
    for i in range(n):
        ln = HEAD[i] if i < len(HEAD) else int(rng.integers(30, 160))
        at = int(rng.integers(0, len(genome) - ln + 1))
        s = genome[at:at + ln]
        if rng.integers(0, 2):
            s = "".join(comp[c] for c in reversed(s))
        s = list(s)
        for j in range(len(s)):                       # a few N and lower-case letters, as read files have them
            u = rng.random()
            if u < 0.01:
                s[j] = "N"
            elif u < 0.05:
                s[j] = s[j].lower()
        out.append("".join(s))
    return out


def write_inputs():
    rng = np.random.default_rng(20201)
    genome = "".join("ACGT"[x] for x in rng.integers(0, 4, GENOME))
    fq = reads(rng, genome, 101)
    with open(os.path.join(HERE, "tenx_reads.fq"), "w") as f:
        for i, s in enumerate(fq):
            f.write("@r%d barcode\n%s\n+\n%s\n" % (i + 1, s, "I" * len(s)))
    fa = reads(rng, genome, 100)
    s0 = list(fa[0])                                    # the first line of the file: 17 bases, lower case and N among them
    s0[3] = s0[3].lower(); s0[9] = "N"; s0[20] = "n"
    fa[0] = "".join(s0)
    with open(os.path.join(HERE, "tenx_reads.fa"), "w") as f:
        for i, s in enumerate(fa):
            width = (17, 29, 60)[i % 3]
            f.write(">seq%d text\n" % (i + 1))
            for a in range(0, len(s), width):
                f.write(s[a:a + width] + "\n")
    for name, rs in (("fq", fq), ("fa", fa)):
        assert all(len(s) >= 23 for s in rs[0::2]), name
    assert len(fq) % 2 == 1
    # the device parser hands complete records on at the ends of its text windows; with the smallest window, 4 KiB, both files are
    # cut after an odd and after an even number of records (tests/test_gpu_modutils_x.py runs them that way)
    for ext in ("fq", "fa"):
        assert {n % 2 for n in window_edges(open(os.path.join(HERE, "tenx_reads." + ext), "rb").read(), ext, 4096)} == {0, 1}, ext


def window_edges(text, ext, window):
    """complete records before every multiple of `window` bytes inside the text: FASTQ by its lines, FASTA by its record starts less the open one"""
    cuts = [text[:e] for e in range(window, len(text), window)]
    return [p.count(b"\n") // 4 if ext == "fq" else p.count(b"\n>") for p in cuts]


def main():
    assert os.path.exists(MU), "needs oracle/_ref/modutils_ref (only buildable where the reference tree exists)"
    write_inputs()
    tmp = tempfile.mkdtemp()
    try:
        for ext in ("fq", "fa"):
            shutil.copy(os.path.join(HERE, "tenx_reads." + ext), tmp)
        for tag, (B, k, w, s) in TAGS.items():
            for ext in ("fq", "fa"):
                base = "tenx_%s_%s" % (tag, ext)
                cmd = [MU, "-c", str(B), str(k), str(w), str(s), "-x", "tenx_reads." + ext, "-s"] + [str(c) for c in COPY] + \
                      ["-sM", str(COPY_M), "-H", base + ".hist.txt", "-wt", base + ".dump.txt", "-w", base + ".mod"]
                r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
                assert r.returncode == 0, (cmd, r.returncode, r.stderr[-2000:])
                out = strip_timing(r.stdout)
                open(os.path.join(tmp, base + ".stdout.txt"), "w").write(out)
                last = out.strip().splitlines()[-1].split()
                tallies = [int(last[last.index(c) + 1]) for c in ("copy0", "copy1", "copy2", "copyM")]
                assert all(tallies), (base, tallies)               # all four classes
                a = subprocess.run([MU, "-c", str(B), str(k), str(w), str(s), "-a", "tenx_reads." + ext], capture_output=True, text=True, cwd=tmp)
                added = lambda t: [l for l in t.splitlines() if l.startswith("added ")][0]
                assert added(a.stdout) != added(r.stdout)          # the barcodes would have hashed
                for suffix in (".stdout.txt", ".hist.txt", ".dump.txt", ".mod"):
                    src = os.path.join(tmp, base + suffix)
                    assert os.path.getsize(src) < LIMIT, (src, os.path.getsize(src))
                    shutil.copy(src, HERE)
                print(base, added(r.stdout), "| -a:", added(a.stdout), "|", tallies)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
