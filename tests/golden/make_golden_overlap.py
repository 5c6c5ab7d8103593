#!/usr/bin/env python3
"""Generate tests/golden/ovl_<tag>* by running the REFERENCE ITSELF (oracle/_ref/modutils_ref, modasm_ref): a read set of about 40 reads on
which modasm's overlap passes -- findOverlaps (modasm.c:314-418) behind -o1 / -o2 / -b (markBadReads, 1266-1322) / -c (markContained,
1370-1394) -- take every branch, and on which their outcome depends on the order of the commands.  The outputs are data: inputs and the
reference's answers.  Re-run with:  python tests/golden/make_golden_overlap.py

  ovl_<tag>_src.fa, ovl_<tag>_reads.fa, ovl_<tag>_src.mod     (modutils -c 20 k w 17 -a .. -s 1 2 3 -w ..; modasm -m .. -f .. -w ovl_<tag>)
  ovl_<tag>.mod / .readset                                    the ingested set
  ovl_<tag>.<name>.stdout.txt                                 modasm -r ovl_<tag> <the commands of SEQUENCES[name]>, timing lines stripped
  ovl_<tag>_BC.mod / .readset                                 written by the sequence "bc" (-b -c ... -w): the flags in a file
  ovl_<tag>.sequences.json                                    name -> the commands, for the tests
"""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from modimizer_amd import fasta, synth     # noqa: E402
from oracle import pyoracle as po          # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")
MU, MA = os.path.join(REFDIR, "modutils_ref"), os.path.join(REFDIR, "modasm_ref")
assert os.path.exists(MU) and os.path.exists(MA), "needs oracle/_ref (only buildable where the reference's sources are)"

TAGS = {"k19d8": (19, 8)}
BITS = 20
BAD_REPEAT, BAD_ORDER10, BAD_ORDER1, BAD_NOMATCH, BAD_LOWHIT, BAD_LOWCOPY1 = 1, 2, 4, 8, 16, 32      # modasm.c:38-45


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


def make_inputs(k, w):
    """(source names, source sequences, read names, reads).  Reads are numbered from 1 in the reference's output, in file order."""
    g = synth.iid_bases(30000, 6262)
    src = [("chr", g), ("dup", g[2000:3000]), ("trip1", g[5000:5500]), ("trip2", g[5000:5500])]      # depth 1 -> copy 1, 2 -> copy 2, 3 -> copy M
    cat = np.concatenate
    oh = po.Hasher(k, w, 17)
    mods = lambda s: set(int(x) for x in oh.scan(s)[0])

    def end_sharing(anchor, start, n):
        """the end e for which g[start:e] shares exactly n mods with `anchor` (which lies behind start)"""
        for e in range(start + 700, start + 1200):
            if len(mods(g[start:e]) & mods(anchor)) == n:
                return e
        raise AssertionError("no end shares %d mods" % n)

    reads = []
    add = lambda name, s: reads.append((name, s))
    # region A: tiling reads on both strands, a contained read, three identical reads, a tandem read
    add("tile1", g[6000:8500])
    add("tile2_rc", rc(g[7400:9900]))
    add("tile3", mutate(g[8600:11000], 0.01, 1))
    add("inside_tile1", g[6500:7400])                            # contained, same strand
    add("same1", g[9000:10500]); add("same2", g[9000:10500]); add("same3", g[9000:10500])
    add("tile4_rc", rc(g[10200:12000]))
    add("inside_tile4_rc", g[10500:11400])                       # contained, other strand: never reported (modasm.c:386)
    add("tile5", g[11200:12800])
    # region B: a rearranged read under eleven others: -b's ">= 10" line
    a = 14000
    add("rearranged10", cat([g[a + 700:a + 1400], g[a:a + 700]]))
    for i in range(11):
        add("cover10_%d" % i, g[a - 50 * i:a + 1400 + 50 * (10 - i)])
    add("tandem", cat([g[7000:7500], g[7000:7500]]))             # every copy-1 mod twice: nRepeatMod, badRepeat; after tile1, before its other partners' turn in -b
    # region C: a rearranged read under three others: "multiple"
    a = 17200
    add("cover2_0", g[a - 200:a + 1700])
    add("rearranged2", cat([g[a + 800:a + 1600], g[a:a + 800]]))
    add("cover2_1", rc(g[a - 100:a + 1800]))
    add("cover2_2", g[a:a + 1900])
    # region D: an inverted segment, one partner: flip; "single"
    a = 20600
    add("inverted_mid", cat([g[a:a + 1000], rc(g[a + 1000:a + 1400]), g[a + 1400:a + 2200]]))
    add("cover1", g[a - 100:a + 2300])
    # region E: most of the read inverted against its partner: minus majority with some plus, which the reference calls GOOD
    a = 23600
    add("mostly_inverted", cat([g[a:a + 400], rc(g[a + 400:a + 1600])]))
    add("partner_of_mostly", g[a:a + 1600])
    # region F: pairs that share exactly three mods (listed) and exactly two (not listed)
    p3, p2 = g[26000:27000], g[28500:29500]
    add("anchor3", p3)
    s3 = 25150; e3 = end_sharing(p3, s3, 3)
    add("shares3", g[s3:e3])
    add("anchor2", p2)
    s2 = 27700; e2 = end_sharing(p2, s2, 2)
    add("shares2", g[s2:e2])
    assert len(mods(g[s3:e3]) & mods(p3)) == 3 and len(mods(g[s2:e2]) & mods(p2)) == 2
    # reads that match nothing
    add("junk", synth.iid_bases(1500, 777))                      # no hit: badNoMatch, badLowHit
    add("copy2_only", g[2100:2900])                              # hits, none of copy 1: badNoMatch, badLowCopy1
    add("short", g[100:110])
    add("tile6_last", mutate(g[12500:13400], 0.02, 2))
    for n, s in reads:
        assert n in ("short",) or 700 <= len(s) <= 3000, (n, len(s))
    return [n for n, _ in src], [s for _, s in src], [n for n, _ in reads], [s for _, s in reads]


def read_flags(stem):
    """(bad[1..], contained[1..]) of <stem>.readset (modasm.c:30-57: 72-byte records, bad at byte 24, contained at byte 32)"""
    raw = gzip.open(os.path.join(HERE, stem + ".readset")).read()
    n_max = int.from_bytes(raw[16 + 24:16 + 28], "little")
    at = 16 + 32
    bad = [raw[at + 72 * i + 24] for i in range(n_max)]
    con = [int.from_bytes(raw[at + 72 * i + 32:at + 72 * i + 36], "little", signed=True) for i in range(n_max)]
    return bad, con


RH = re.compile(r"^RH\t(\d+)\tlen (\d+)\t(BAD|GOOD)\t\+ (-?\d+)\t- (-?\d+)\tbadOrder (\d+)\t(CONTAINED|OVERLAP)$")
RR = re.compile(r"^RR +(\d+)\tlen (\d+)\tnHit +(\d+)\tnMiss +(\d+)\tnCpy (\d+) (\d+) (\d+) (\d+)\tnRepeatMod (\d+)\tnGood +(\d+)\tnBad +(\d+)$")


def gen(tag, k, w):
    sn, ss, rn, rr = make_inputs(k, w)
    stem = "ovl_%s" % tag
    no = {name: i + 1 for i, name in enumerate(rn)}
    n = len(rn)
    fasta.write_fasta(os.path.join(HERE, stem + "_src.fa"), sn, ss)
    fasta.write_fasta(os.path.join(HERE, stem + "_reads.fa"), rn, rr)
    run([MU, "-c", str(BITS), str(k), str(w), "17", "-a", stem + "_src.fa", "-s", "1", "2", "3", "-w", stem + "_src.mod"])
    run([MA, "-m", stem + "_src.mod", "-f", stem + "_reads.fa", "-w", stem])
    seqs = {"o2_1": ["-o2", "1"], "o2_3": ["-o2", "3"]}
    for i in range(1, n + 1):
        seqs["o1_%d" % i] = ["-o1", str(i)]
    seqs["bc"] = ["-b", "-c", "-o2", "1", "-o1", str(no["cover10_3"]), "-o1", str(no["inside_tile1"]), "-w", stem + "_BC"]
    seqs["cbc"] = ["-c", "-b", "-c", "-o2", "2"]
    seqs["b_S"] = ["-b", "-S"]
    out = {}
    for name, cmd in seqs.items():
        out[name] = strip_timing(run([MA, "-r", stem] + cmd))
    seqs["rbc"] = ["-o2", "1"]                                    # read from ovl_<tag>_BC: the flags survive the file
    out["rbc"] = strip_timing(run([MA, "-r", stem + "_BC", "-o2", "1"]))
    for name, text in out.items():
        open(os.path.join(HERE, "%s.%s.stdout.txt" % (stem, name)), "w").write(text)
    json.dump({"nReads": n, "names": rn, "sequences": seqs, "reads_from": {"rbc": stem + "_BC"}},
              open(os.path.join(HERE, stem + ".sequences.json"), "w"), indent=1)

    # ---- the fixture holds what it is for, by the reference's own output ----
    rh = {i: [RH.match(l).groups() for l in out["o1_%d" % i].splitlines() if l.startswith("RH")] for i in range(1, n + 1)}
    rr1 = {i: RR.match([l for l in out["o1_%d" % i].splitlines() if l.startswith("RR")][0]).groups() for i in range(1, n + 1)}
    allrh = [(i,) + t for i in rh for t in rh[i]]
    P = lambda t: (int(t[4]), int(t[5]), int(t[6]))              # nPlus, nMinus, badOrder of (x, iy, len, verdict, +, -, badOrder, kind)
    assert any(P(t)[0] > 0 and P(t)[1] == 0 and t[3] == "GOOD" for t in allrh if t[0] != int(t[1]))        # an overlap in each strand
    assert any(P(t)[0] == 0 and P(t)[1] > 0 and t[3] == "GOOD" for t in allrh)
    assert any(t[7] == "CONTAINED" for t in allrh)
    assert any(t[0] == no["inside_tile1"] and int(t[1]) == no["tile1"] and t[7] == "CONTAINED" for t in allrh)
    assert any(t[3] == "BAD" and P(t)[2] > 0 and P(t)[1] == 0 for t in allrh)                              # BAD from order alone
    assert any(t[3] == "BAD" and P(t)[0] > P(t)[1] > 0 for t in allrh)                                     # BAD from flip
    assert any(t[3] == "GOOD" and P(t)[1] > P(t)[0] > 0 for t in allrh)                                    # minus majority, mixed: GOOD
    assert any(t[0] == no["mostly_inverted"] and int(t[1]) == no["partner_of_mostly"] and t[3] == "GOOD" and P(t)[1] > P(t)[0] > 0 for t in allrh)
    # three identical reads: equal nHit, listed in arrival order
    for x in ("same1", "tile3"):
        ys = [int(t[0]) for t in rh[no[x]]]
        three = [y for y in ys if y in (no["same1"], no["same2"], no["same3"])]
        assert three == [no["same1"], no["same2"], no["same3"]], (x, ys)
        if x == "tile3":
            assert len({(t[3], t[4], t[5]) for t in rh[no[x]] if int(t[0]) in three}) == 1
    # exactly two shared mods: absent; exactly three: present
    assert not any(int(t[0]) == no["shares2"] for t in rh[no["anchor2"]]) and not any(int(t[0]) == no["anchor2"] for t in rh[no["shares2"]])
    assert [P(t) for t in allrh if t[0] == no["anchor3"] and int(t[1]) == no["shares3"]] == [(3, 0, 0)]
    assert [P(t) for t in allrh if t[0] == no["shares3"] and int(t[1]) == no["anchor3"]] == [(3, 0, 0)]
    # repeats: the read does not list itself
    assert int(rr1[no["tandem"]][8]) > 0 and not any(int(t[0]) == no["tandem"] for t in rh[no["tandem"]]) and len(rh[no["tandem"]]) > 0
    assert any(int(t[0]) == no["tile1"] for t in rh[no["tile1"]])                                          # ... and a read without repeats does
    # the flags after -b -c
    bad, con = read_flags(stem + "_BC")
    assert bad[0] == 0 and len(bad) == n + 1
    assert bad[no["junk"]] == BAD_NOMATCH | BAD_LOWHIT and bad[no["copy2_only"]] == BAD_NOMATCH | BAD_LOWCOPY1
    assert bad[no["tandem"]] & BAD_REPEAT and bad[no["rearranged10"]] & BAD_ORDER10 and bad[no["rearranged2"]] & BAD_ORDER1
    assert con[no["inside_tile1"]] == no["tile1"] and sum(1 for c in con if c) >= 2
    mb = [int(re.match(r"MB  (\d+) with", l).group(1)) for l in out["bc"].splitlines() if l.startswith("MB")]
    assert len(mb) == 3 and all(v > 0 for v in mb), mb
    assert [l for l in out["bc"].splitlines() if l.startswith("MC")]
    # the order dependence: -o2 1 before and after -b
    before = [l for l in out["o2_1"].splitlines() if l.startswith("RR")]
    after = [l for l in out["bc"].splitlines() if l.startswith("RR")][:n]
    assert len(before) == len(after) == n and before != after
    assert [l for l in out["rbc"].splitlines() if l.startswith("RR")] == after                            # and the flags survive the file
    assert "RS bad" in out["b_S"] and not re.search(r"^RS bad 0 ", out["b_S"], re.M)
    sizes = {f: os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith(stem)}
    assert max(sizes.values()) < 150 * 1024, sizes
    print(stem, "reads", n, "MB", mb, "| differing RR lines", sum(x != y for x, y in zip(before, after)),
          "| files", len(sizes), "largest", max(sizes.values()), "total", sum(sizes.values()))


if __name__ == "__main__":
    for tag, (k, w) in TAGS.items():
        gen(tag, k, w)
