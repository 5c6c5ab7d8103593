#!/usr/bin/env python3
"""Generate tests/golden/clean_<tag>.* by running the REFERENCE ITSELF (oracle/_ref/modutils_ref, modasm_ref): a small read set on which
modasm -C (cleanMods, modasm.c:514-555) sets all three kinds of flag and -P (readProperties, modasm.c:912-952) prints every kind of line.
The asm_* fixtures of make_golden.py cannot show either: no read of theirs holds a mod twice.  The outputs are data: inputs and the
reference's answers.  Re-run with:  python tests/golden/make_golden_clean.py

  clean_<tag>_src.fa      the sequences the source set is made of        (modutils -c 20 k w 17 -a .. -s 1 2 3 -w clean_<tag>_src.mod)
  clean_<tag>_reads.fa    the reads                                      (modasm -m clean_<tag>_src.mod -f .. -w clean_<tag>)
  clean_<tag>.mod/.readset        the ingested set
  clean_<tag>_C.mod/.readset, clean_<tag>.stdout.txt                     (modasm -r clean_<tag> -C -P -w clean_<tag>_C: the -C line, then -P's)
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from modimizer_amd import fasta, synth     # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")
MU, MA = os.path.join(REFDIR, "modutils_ref"), os.path.join(REFDIR, "modasm_ref")
assert os.path.exists(MU) and os.path.exists(MA), "needs oracle/_ref (only buildable where the reference's sources are)"

TAGS = {"k19d8": (19, 8)}
BITS = 20


def strip_timing(text):
    """drop the getrusage lines (utils.c:187-193): timing noise (as make_golden.py does)"""
    return "\n".join(l for l in text.splitlines() if not l.startswith("user\t") and "resources used" not in l
                     and not l.startswith("total resources")) + "\n"


def run(cmd, cwd=HERE):
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    return r.stdout


def rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def mutate(s, rate, seed):
    r = np.random.default_rng(seed)
    s = s.copy()
    m = r.random(len(s)) < rate
    s[m] = (s[m] + 1 + r.integers(0, 3, int(m.sum()))) & 3
    return s


def make_inputs():
    """(source names, source sequences, read names, reads).  Reads are numbered from 1 in the reference's output, in file order."""
    g = synth.iid_bases(16000, 5150)
    src = [("chr", g), ("dup", g[2000:3000]), ("trip1", g[5000:5500]), ("trip2", g[5000:5500])]      # depth 1 -> copy 1, 2 -> copy 2, 3 -> copy M
    cat = np.concatenate
    reads = [
        ("plain1", g[9000:11500]),
        ("plain2_rc", rc(g[9200:12000])),
        ("plain3", mutate(g[8800:11800], 0.01, 1)),
        ("plain4", g[9500:11000]),
        ("across_depths", g[10500:13500]),                       # from a region that five reads cover into one that it alone does: minor variants
        ("tandem_mid", cat([g[500:1300], g[500:1300]])),         # every mod twice in one orientation: repeats, n2Tan
        ("copy2_and_M", g[1800:5700]),
        ("fwd_and_rev", cat([g[6000:6800], rc(g[6000:6800])])),  # every mod once forward, once reverse: n2Rev
        ("junk", synth.iid_bases(1500, 777)),                    # hits nothing
        ("thrice", cat([g[7000:7600]] * 3 + [g[8000:8400], g[8000:8400], rc(g[8000:8400])])),      # MT lines, more than five: an RM line that lists the (2, 1) mods too
        ("thrice_short", cat([rc(g[13600:13650])] * 4)),          # a few MT lines, no RM line
        ("plain5", mutate(g[12500:15500], 0.02, 2)),
        ("short", g[100:110]),
        ("plain6_rc", rc(g[0:2500])),
        ("tandem_last", cat([g[14500:15300], g[14500:15300]])),  # LAST: cleanMods never looks at it (modasm.c:522-523)
    ]
    return [n for n, _ in src], [s for _, s in src], [n for n, _ in reads], [s for _, s in reads]


def c_counts(text):
    m = re.search(r"^set (\d+) repeated, (\d+) internal, (\d+) minor_variant mods$", text, re.M)
    assert m, text[:400]
    return tuple(int(x) for x in m.groups())


def gen(tag, k, w):
    sn, ss, rn, rr = make_inputs()
    stem = "clean_%s" % tag
    fasta.write_fasta(os.path.join(HERE, stem + "_src.fa"), sn, ss)
    fasta.write_fasta(os.path.join(HERE, stem + "_reads.fa"), rn, rr)
    run([MU, "-c", str(BITS), str(k), str(w), "17", "-a", stem + "_src.fa", "-s", "1", "2", "3", "-w", stem + "_src.mod"])
    run([MA, "-m", stem + "_src.mod", "-f", stem + "_reads.fa", "-w", stem])
    out = strip_timing(run([MA, "-r", stem, "-C", "-P", "-w", stem + "_C"]))
    open(os.path.join(HERE, stem + ".stdout.txt"), "w").write(out)

    # ---- the fixture holds what it is for, by the reference's own output ----
    n_rep, n_int, n_minor = c_counts(out)
    assert n_rep > 0 and n_int > 0 and n_minor > 0, (n_rep, n_int, n_minor)
    read_lines = {}
    for l in out.splitlines():
        m = re.match(r"READ (\d+) n (\d+) n2Tan (\d+) n2Rev (\d+) nMoreTan (\d+) nMoreRev (\d+)$", l)
        if m:
            v = [int(x) for x in m.groups()]
            read_lines[v[0]] = dict(n=v[1], n2Tan=v[2], n2Rev=v[3], nMoreTan=v[4], nMoreRev=v[5])
    assert sorted(read_lines) == list(range(1, len(rn) + 1))                       # -P looks at every read, the last included
    no = {name: i + 1 for i, name in enumerate(rn)}
    assert no["tandem_last"] == len(rn) and 1 < no["tandem_mid"] < len(rn)
    assert read_lines[no["tandem_mid"]]["n2Tan"] > 5 and read_lines[no["tandem_last"]]["n2Tan"] > 5
    assert read_lines[no["fwd_and_rev"]]["n2Rev"] > 5
    assert read_lines[no["thrice"]]["nMoreTan"] > 5 and read_lines[no["thrice"]]["nMoreRev"] > 0
    assert 0 < read_lines[no["thrice_short"]]["nMoreTan"] <= 5
    assert read_lines[no["junk"]]["n"] == 0
    mt = [l for l in out.splitlines() if l.startswith("MT i %d h " % no["thrice"])]
    assert len(mt) == read_lines[no["thrice"]]["nMoreTan"] and all(l.endswith(" count 3") for l in mt)
    assert any(l.startswith("MT i %d h " % no["thrice_short"]) and l.endswith(" count 4") for l in out.splitlines())
    rm = [l for l in out.splitlines() if l.startswith("RM ")]
    assert len(rm) == 1 and rm[0].startswith("RM %d nMoreTan %d " % (no["thrice"], len(mt)))
    assert len(rm[0].split()) - 4 == len(mt) + read_lines[no["thrice"]]["nMoreRev"]      # the RM line lists the (2, 1) mods as well
    # the last read is not processed by -C: the same reads with the last one moved to the front set more repeat flags
    with tempfile.TemporaryDirectory() as d:
        order = [len(rn) - 1] + list(range(len(rn) - 1))
        fasta.write_fasta(os.path.join(d, "r.fa"), [rn[i] for i in order], [rr[i] for i in order])
        run([MA, "-m", os.path.join(HERE, stem + "_src.mod"), "-f", "r.fa", "-w", "moved"], cwd=d)
        moved = c_counts(run([MA, "-r", "moved", "-C"], cwd=d))
    assert moved[0] > n_rep, (moved, n_rep)
    print(stem, "-C:", (n_rep, n_int, n_minor), "last read first:", moved, "| MT lines", sum(l.startswith("MT ") for l in out.splitlines()),
          "| sizes", {e: os.path.getsize(os.path.join(HERE, stem + e)) for e in ("_src.fa", "_reads.fa", "_src.mod", ".mod", ".readset", "_C.mod", "_C.readset", ".stdout.txt")})


if __name__ == "__main__":
    for tag, (k, w) in TAGS.items():
        gen(tag, k, w)
