#!/usr/bin/env python3
"""Generate tests/golden/rdna_<tag>* by running the REFERENCE ITSELF (oracle/_ref/modutils_ref, modasm_ref): a long-read set over a tandem array on
which modasm's rDNA passes -- refFlag (modasm.c:752-860) behind -R, testMods (595-748) behind -T, resetBits (864-908) behind -rb -- take every
branch.  The outputs are data: inputs and the reference's answers.  Re-run with:  python tests/golden/make_golden_rdna.py

  rdna_<tag>_src.fa, rdna_<tag>_reads.fa.gz, rdna_<tag>_src.mod   (modutils -c 20 k w 17 -a .. -s 1 2 3 -w ..; modasm -m .. -f .. -w rdna_<tag>)
  rdna_<tag>_ref.fa, _ref2.fa, _refN.fa                        reference sequences for -R: the unit with flanks that miss; a variant unit; one with an N
  rdna_<tag>.mod / .readset                                    the ingested set
  rdna_<tag>.<name>.json.gz                                    modasm -r rdna_<tag> <the commands of SEQUENCES[name]>: stdout (timing lines stripped),
                                                               the YY-TEST<n> and ZZ-TEST<n> files it wrote, its exit status and last stderr line
  rdna_<tag>_W.mod / .readset                                  written by the sequence "w" (-R -C -T -w): otherFlags in a file, ModInfo not
  rdna_<tag>_X.mod / .readset                                  written by the sequence "example": what examples/rdna_file.c writes
  rdna_<tag>.sequences.json                                    name -> the commands, for the tests

The thresholds of -R are hard-coded (core: depth 2751 .. 4750), so the array's unit is short (96 bases, w = 8 <= k = 19) and a read of c copies adds c to
the depth of the unit's mods: 48 reads of 52 .. 80 units reach it.  Variant units give var mods; half of the reads are reverse-complemented; three reads
are too short for 400 core hits (m200 <= n200).

An N in the reference file: modasm.c:159 maps N to 0 only when -f ran earlier in the process; after -r the iterator hashes a base 4 that its tables do
not have.  The library reads N as base 0 everywhere.  The N of _refN.fa replaces a base that no read has as A there and lies in a flank, far from the
unit, so both readings give the same hits: asserted below by running -R on the file and on its copy with the N written as A (the `-r stem -R` case)."""
import gzip
import json
import os
import re
import shutil
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
UNIT, SLOTS = 96, 150
LIMIT = 512 * 1024


def strip_timing(text):
    return "\n".join(l for l in text.splitlines() if not l.startswith("user\t") and "resources used" not in l
                     and not l.startswith("total resources")) + "\n"


def rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def snp(u, at, by=1):
    v = u.copy(); v[at] = (v[at] + by) & 3
    return v


def make_inputs(unit=UNIT):
    """(source names, sources, read names, reads, {reference file suffix: (names, sequences, the place of an N or None)}); a longer unit makes the same
    design with more mods per unit and more hits per read (tools/rdna_probe.py)"""
    rng = np.random.default_rng(4242)
    u = synth.iid_bases(unit, 9191)
    seg = synth.iid_bases(30, 9292)                                   # a segment that sits at two different offsets of the unit: its mods get two rDNApos
    types, place = {}, {}
    for j in range(36):                                               # variants that stand at one slot: a read holds their mods once, so -C leaves them alone
        types["v%d" % j] = snp(u, 5 + (j * 7) % 86, 1 + j % 3); place["v%d" % j] = (4 * j + 2,)
    types["far"] = snp(u, 47, 3); place["far"] = (9, 141)           # never twice in one read, on either side of the mods between: a split
    types["d0"] = snp(u, 33, 3); place["d0"] = (40, 59)              # twice in most reads that hold it
    types["d1"] = snp(u, 77, 1); place["d1"] = (100, 101)
    types["segA"] = np.concatenate([u[:20], seg, u[20:]]); place["segA"] = (35, 92)
    types["segB"] = np.concatenate([u[:70], seg, u[70:]]); place["segB"] = (64, 119)
    slots = ["u"] * SLOTS
    for t, at in place.items():
        for s in at:
            assert slots[s] == "u", (t, s)
            slots[s] = t
    types["u"] = u
    slots_b = ["u" if t.startswith("v") and int(t[1:]) % 4 != 0 else t for t in slots]      # the second haplotype, two reads in three, lacks three quarters of the single variants: poor partners
    left, right = synth.iid_bases(400, 9393), synth.iid_bases(400, 9494)
    units = [types[t] for t in slots]
    start = np.concatenate([[0], np.cumsum([len(x) for x in units])])
    array = np.concatenate(units)
    array_b = np.concatenate([types[t] for t in slots_b])
    assert len(array_b) == len(array)
    private = snp(u, 50, 2)                                          # a variant that one read alone carries: its mods are partners with n == 1
    src = [("array", np.concatenate([left, array, right])), ("private", np.concatenate([u[-30:], private, u[:30]]))]
    reads = []
    for i in range(48):
        n = int(rng.integers(52, 81)); a = int(rng.integers(0, SLOTS - n + 1))
        s = (array_b if i % 3 != 0 else array)[start[a]:start[a + n]].copy()
        if i == 7:                                                    # the private variant in place of a unit in the middle of this read
            j = a + n // 2
            while slots[j] != "u":
                j += 1
            s[start[j] - start[a]:start[j + 1] - start[a]] = private
        reads.append(("r%02d_%d_%d%s" % (i, a, n, "_rc" if i % 2 else ""), rc(s) if i % 2 else s))
    for i, (a, n) in enumerate([(10, 20), (60, 30), (100, 33)]):      # fewer than 400 core hits: m200 <= n200
        s = array[start[a]:start[a + n]]
        reads.append(("short%d_%d_%d" % (i, a, n), rc(s) if i == 1 else s))
    reads.append(("flank", np.concatenate([left, array[:start[8]]])))             # few core hits, flank mods
    reads.append(("junk", synth.iid_bases(3000, 9595)))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    ref = np.concatenate([synth.iid_bases(150, 9696), u, u, u[:40], synth.iid_bases(150, 9797)])      # flanks whose mods miss
    ref2 = np.concatenate([types["v4"], types["segA"], u[:30]])
    n_at = 60                                                         # in the left flank of ref: its k-mers are in no read whichever base stands there
    refs = {"_ref": (["unit"], [ref], None), "_ref2": (["variants"], [ref2], None), "_refN": (["unit_with_N"], [ref], n_at)}
    return [n for n, _ in src], [s for _, s in src], [n for n, _ in reads], [s for _, s in reads], refs


def write_ref(path, names, seqs, n_at):
    fasta.write_fasta(path, names, seqs)
    if n_at is not None:
        lines = open(path).read().split("\n")
        body = list("".join(lines[1:]))
        body[n_at] = "N"
        open(path, "w").write(lines[0] + "\n" + "".join(body) + "\n")


def run_seq(stem, cmd, keep=()):
    """the reference on `cmd` in a directory of its own (it writes YY-TEST<n> / ZZ-TEST<n> where it runs)"""
    d = tempfile.mkdtemp()
    try:
        for f in os.listdir(HERE):
            if f.startswith(stem.split(".")[0]) and f.endswith((".fa", ".mod", ".readset")):
                os.symlink(os.path.join(HERE, f), os.path.join(d, f))
        r = subprocess.run([MA] + cmd, capture_output=True, text=True, cwd=d)
        out = {"stdout": strip_timing(r.stdout), "rc": r.returncode, "stderr": (r.stderr.strip().splitlines() or [""])[-1], "YY": {}, "ZZ": {}}
        for f in sorted(os.listdir(d)):
            m = re.match(r"(YY|ZZ)-TEST(\d+)$", f)
            if m:
                out[m.group(1)][m.group(2)] = open(os.path.join(d, f)).read()
        for f in keep:
            shutil.copy(os.path.join(d, f), os.path.join(HERE, f))
        return out
    finally:
        shutil.rmtree(d)


def read_other_flags(path):
    raw = gzip.open(path).read()
    n_max = int.from_bytes(raw[40:44], "little")
    return [raw[48 + 72 * i + 25] for i in range(n_max)]


def gen(tag, k, w):
    sn, ss, rn, rr, refs = make_inputs()
    stem = "rdna_%s" % tag
    for f in os.listdir(HERE):
        if f.startswith(stem):
            os.remove(os.path.join(HERE, f))
    fasta.write_fasta(os.path.join(HERE, stem + "_src.fa"), sn, ss)
    reads_fa = os.path.join(HERE, stem + "_reads.fa")                   # committed gzipped (the reference reads it through zlib): 320 KiB of text otherwise
    fasta.write_fasta(reads_fa, rn, rr)
    with gzip.GzipFile(reads_fa + ".gz", "wb", mtime=0) as f:
        f.write(open(reads_fa, "rb").read())
    os.remove(reads_fa)
    for suffix, (names, seqs, n_at) in refs.items():
        write_ref(os.path.join(HERE, stem + suffix + ".fa"), names, seqs, n_at)
    run = lambda cmd: subprocess.run(cmd, capture_output=True, text=True, cwd=HERE, check=True).stdout
    run([MU, "-c", str(BITS), str(k), str(w), "17", "-a", stem + "_src.fa", "-s", "1", "2", "3", "-w", stem + "_src.mod"])
    run([MA, "-m", stem + "_src.mod", "-f", stem + "_reads.fa.gz", "-w", stem])
    R, R2, RN = ["-R", stem + "_ref.fa"], ["-R", stem + "_ref2.fa"], ["-R", stem + "_refN.fa"]
    T = ["-T", "2", "400"]
    TC = ["-T", "2751", "4751"]                                       # the core mods
    RB1, RB2, RB3, C = ["-rb", "1"], ["-rb", "2"], ["-rb", "3"], ["-C"]
    # Without -C the unit's own mods are partners on both sides of every mod, so every tested mod is split more than 10 times and gets copy 0: only
    # -rb brings core mods back, and a -T that tests no mod dies (modasm.c:746: arrayDestroy (0)).  With -C the unit's mods are REPEAT and out of it.
    seqs = {
        "R": R,
        "RN": RN,
        "RR2": R + R2 + C + T,
        "T8": R + T + TC + RB1 + TC + RB1 + TC + RB2 + TC + RB3 + RB1 + TC + RB1 + TC + ["-rb", "7"] + RB1 + TC,      # RUN 1 .. 8
        "CT4": R + C + T + ["-T", "10", "30"] + T + T,
        "CTR2T": R + C + T + R2 + T,                                  # a second -R between two -T
        "Tcore": R + TC,
        "C_S": R + C + T + ["-S"] + RB2 + ["-S"],
        "rb1": R + RB1 + TC + ["-S"],
        "rb3": R + RB3 + ["-S"],
        "w": R + C + T + ["-w", stem + "_W"],
        "example": R + T + TC + RB2 + ["-w", stem + "_X"],           # examples/rdna_file.c
        "noR": T,                                                     # dies: need to run -R first
        "none": R + ["-T", "5000", "6000"],                           # dies at its end: no mod tested
    }
    if os.environ.get("RDNA_PROBE"):
        for name, cmd in seqs.items():
            o = run_seq(stem, ["-r", stem] + cmd)
            print(name, o["rc"], o["stderr"][:60]); print("   " + "\n   ".join(l for l in o["stdout"].splitlines() if l.startswith(("RUN", "total", "  n", "set", "reset"))))
        return
    out = {}
    for name, cmd in seqs.items():
        keep = [cmd[-1] + ".mod", cmd[-1] + ".readset"] if "-w" in cmd else []
        out[name] = run_seq(stem, ["-r", stem] + cmd, keep)
    seqs["rW"] = T                                                    # read back from rdna_<tag>_W: the flags survive, ModInfo does not
    out["rW"] = run_seq(stem, ["-r", stem + "_W"] + T)
    # the N: the same answer as with an A in its place
    path_a = os.path.join(HERE, stem + "_refA.fa")
    open(path_a, "w").write(open(os.path.join(HERE, stem + "_refN.fa")).read().replace("N", "A"))
    as_a = run_seq(stem, ["-r", stem, "-R", stem + "_refA.fa"])
    os.remove(path_a)
    assert as_a["stdout"] == out["RN"]["stdout"] == out["R"]["stdout"], "the N changes the reference's hits: move it"
    for name, o in out.items():
        with gzip.GzipFile(os.path.join(HERE, "%s.%s.json.gz" % (stem, name)), "wb", mtime=0) as f:
            f.write(json.dumps(o, indent=0, sort_keys=True).encode())
    json.dump({"nReads": len(rn), "names": rn, "sequences": seqs, "reads_from": {"rW": stem + "_W"}, "refs": {s: stem + s + ".fa" for s in refs}},
              open(os.path.join(HERE, stem + ".sequences.json"), "w"))

    # ---- the fixture holds what it is for, by the reference's own output ----
    for name, o in out.items():
        assert (o["rc"] != 0) == (name in ("noR", "rW", "none")), (name, o["rc"], o["stderr"], [l for l in o["stdout"].splitlines() if l.startswith("RUN")])
    assert "arrayDestroy" in out["none"]["stderr"]
    assert "need to run -R first" in out["noR"]["stderr"] and "need to run -R first" in out["rW"]["stderr"]
    m = re.search(r"total nRDNAreads (\d+) other reads (\d+)", out["R"]["stdout"])
    assert int(m.group(1)) >= 40 and int(m.group(2)) >= 3, m.groups()                      # reads both with and without isRDNA
    flags = read_other_flags(os.path.join(HERE, stem + "_W.readset"))
    assert sum(flags) == int(m.group(1)) and flags[0] == 0 and set(flags) == {0, 1}
    assert read_other_flags(os.path.join(HERE, stem + ".readset")) == [0] * len(flags)
    m = re.search(r"nOthC (\d+) nOthM (\d+) nOthVcopy>0 (\d+) nOthVcopy0 (\d+) nGoodPos (\d+)", out["R"]["stdout"])
    n_oth = sum(int(x) for x in m.groups()[:4])
    assert 0 < int(m.group(5)) < n_oth, m.groups()                                         # non-ref mods with an averaged and with a -1 rDNApos
    m = re.search(r"nRefC (\d+) nRefM (\d+) nRefVcopy>0 (\d+)", out["R"]["stdout"])
    assert int(m.group(1)) >= 8, m.groups()
    assert out["RR2"]["stdout"].count("total nRDNAmods") == 2
    zz = "".join(out["T8"]["ZZ"].values()) + "".join(out["CT4"]["ZZ"].values())
    Z = re.compile(r"^i (\d+) depth (\d+) m (\d+) depth (\d+) ([+-]) count (\d+) min (\d+) at (-?\d+) max (\d+) at (-?\d+)$", re.M)
    rows = [(int(a), int(b), int(c), int(d), s, int(n), int(v1), int(x1), int(v2), int(x2)) for a, b, c, d, s, n, v1, x1, v2, x2 in Z.findall(zz)]
    assert len(rows) == zz.count("\n") and rows
    assert any(r[4] == "+" for r in rows) and any(r[4] == "-" for r in rows)
    assert any(r[5] == 1 and r[6] >= 10 for r in rows), "no n == 1 partner under a cover of at least 10"
    runs = [re.search(r"^RUN (\d+) tested (\d+) mods and zeroed (\d+) bad>good (\d+) split (\d+) LD$", l).groups() for l in out["T8"]["stdout"].splitlines() if l.startswith("RUN")]
    assert [int(r[0]) for r in runs] == list(range(1, 9)) and int(runs[0][1]) > 0, runs
    assert [int(l.split()[1]) for l in out["CT4"]["stdout"].splitlines() if l.startswith("RUN")] == list(range(1, 5))
    yy = "".join(out["T8"]["YY"].values()) + "".join(out["CT4"]["YY"].values())
    Y = re.compile(r"^TEST (\d+) depth (\d+) nGood (\d+) nMod2 (\d+) nBadLD (\d+) nSplit (\d+)$", re.M)
    ys = [tuple(int(x) for x in t) for t in Y.findall(yy)]
    assert any(t[2] for t in ys) and any(t[3] for t in ys) and any(t[4] for t in ys) and any(t[5] for t in ys), "nGood, nMod2, nBadLD, nSplit all non-zero somewhere"
    assert "BADLD" in yy
    allruns = runs + [re.search(r"^RUN (\d+) tested (\d+) mods and zeroed (\d+) bad>good (\d+) split (\d+) LD$", l).groups() for l in out["CT4"]["stdout"].splitlines() if l.startswith("RUN")]
    assert any(int(r[2]) for r in allruns) and any(int(r[3]) for r in allruns) and any(int(r[4]) for r in allruns), allruns
    assert "kept" in out["rb1"]["stdout"] and "kept" in out["rb3"]["stdout"] and "set " in out["C_S"]["stdout"]
    sizes = {f: os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith(stem)}
    assert max(sizes.values()) <= LIMIT, sorted(sizes.items(), key=lambda t: -t[1])[:5]
    print(stem, "reads", len(rn), "runs", runs, "| ZZ rows", len(rows), "| files", len(sizes), "largest", max(sizes.values()), "total", sum(sizes.values()))


if __name__ == "__main__":
    for tag, (k, w) in TAGS.items():
        gen(tag, k, w)
