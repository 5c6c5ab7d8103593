#!/usr/bin/env python3
"""Generate tests/golden/report_* by running the REFERENCE ITSELF (oracle/_ref/modutils_ref, built from the reference tree by
oracle/Makefile): modutils -P (modutils.c:260-273) and -d (modutils.c:65-77) on the existing reads.fa / reads2.fa / ref.fa.
Re-run with:  python tests/golden/make_golden_report.py

Per tag of util.MODUTILS_TAGS (B k w s):
  report_<tag>.paint.txt    stdout of  modutils_ref -o <scratch> -c B k w s -a reads.fa -a reads2.fa -P ref.fa
                            (-a first: only then does -P's dna2indexConv map N to 0, modutils.c:39); the final
                            "total resources used" line dropped
  report_<tag>.paint_reads.txt   the same with -P reads.fa (ref.fa shares no k-mer with the reads: headers only; reads.fa
                            holds every painted case -- hits, a record shorter than k, N, lower case)
  report_<tag>_{a,b,seed,k15}.mod   the other sets, written by modutils_ref -w (gzip, as its fzopen writes them):
                            a = reads.fa only, b = reads2.fa only, seed = reads.fa at seed s + 6, k15 = reads.fa at k = 15
  report_<tag>.depths.txt   the -d file of the same set against those four (-d opens them with fopen: it is given them gunzipped)
Texts above ~100 KB are kept as <name>.digest.json (util.check_dump's form).
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import util  # noqa: E402

MU = os.path.join(ROOT, "oracle", "_ref", "modutils_ref")
OTHERS = ("a", "b", "seed", "k15")
DIGEST_ABOVE = 100_000


def run(cmd, cwd):
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    return r.stdout


def drop_total(text):
    lines = text.splitlines(keepends=True)
    while lines and not lines[-1].startswith("painting ") and not lines[-1].startswith("  "):
        lines.pop()                                     # "total resources used: ..." (modutils.c:279)
    return "".join(lines)


def keep(name, text):
    path = os.path.join(HERE, name)
    dig = path.replace(".txt", ".digest.json")
    for p in (path, dig):
        if os.path.exists(p):
            os.remove(p)
    if len(text) <= DIGEST_ABOVE:
        open(path, "w").write(text)
    else:
        lines = text.splitlines()
        json.dump({"lines": len(lines), "head": lines[:40], "tail": lines[-5:],
                   "sha256": hashlib.sha256(text.encode()).hexdigest(), "bytes": len(text)}, open(dig, "w"), indent=0)
    print(name, len(text), "bytes", "(digest)" if len(text) > DIGEST_ABOVE else "")


def other_params(tag, which):
    B, k, w, s = util.MODUTILS_TAGS[tag]
    return {"a": (B, k, w, s, "reads.fa"), "b": (B, k, w, s, "reads2.fa"),
            "seed": (B, k, w, s + 6, "reads.fa"), "k15": (20, 15, w, s, "reads.fa")}[which]


def main():
    assert os.path.exists(MU), "needs oracle/_ref/modutils_ref (only buildable where the reference tree exists)"
    tmp = tempfile.mkdtemp()
    try:
        for name in ("reads.fa", "reads2.fa", "ref.fa"):
            shutil.copy(os.path.join(HERE, name), tmp)
        for tag, (B, k, w, s) in util.MODUTILS_TAGS.items():
            base = ["-c", str(B), str(k), str(w), str(s), "-a", "reads.fa", "-a", "reads2.fa"]
            keep("report_%s.paint.txt" % tag, drop_total(run([MU, "-o", "log.txt"] + base + ["-P", "ref.fa"], tmp)))
            keep("report_%s.paint_reads.txt" % tag, drop_total(run([MU, "-o", "log.txt"] + base + ["-P", "reads.fa"], tmp)))
            plain = []
            for o in OTHERS:
                b, kk, ww, ss, fa = other_params(tag, o)
                mod = "report_%s_%s.mod" % (tag, o)
                run([MU, "-o", "log.txt", "-c", str(b), str(kk), str(ww), str(ss), "-a", fa, "-w", mod], tmp)
                shutil.copy(os.path.join(tmp, mod), os.path.join(HERE, mod))
                with gzip.open(os.path.join(tmp, mod)) as g:
                    open(os.path.join(tmp, mod + ".plain"), "wb").write(g.read())
                plain.append(mod + ".plain")
                print(mod, os.path.getsize(os.path.join(HERE, mod)), "bytes")
            run([MU, "-o", "log.txt"] + base + ["-d", "depths.txt"] + plain, tmp)
            keep("report_%s.depths.txt" % tag, open(os.path.join(tmp, "depths.txt")).read())
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
