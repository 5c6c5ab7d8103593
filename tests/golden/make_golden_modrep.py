#!/usr/bin/env python3
"""Generate tests/golden/rep_* by running the REFERENCE ITSELF: oracle/_ref/modutils_ref for the sets, and modrep, which oracle/ does not
build: its modrep.c is compiled here into a temporary directory, with the line oracle/Makefile uses for modasm_ref, run, and deleted with
the directory.  Only where the reference's sources are.  modrep opens .mod files with plain fopen, so they are gunzipped into that
directory for it.  The outputs are data: inputs and the reference's answers.  Re-run with:  python tests/golden/make_golden_modrep.py

  rep_<tag>_ref.fa / _ref.mod      one 60 kb iid sequence and its set         (modutils -c 20 k w 17 -a rep_<tag>_ref.fa -w rep_<tag>_ref.mod)
  rep_<tag>_reads.fa               the reads
  rep_<tag>_reads.mod              the second set: the reads but the orphan, then a junk tail that no read holds, so entry max is in no read
  rep_<tag>.stdout.txt / .stderr.txt    modrep -R rep_<tag>_ref.fa ref.raw -s3 rep_<tag>_reads.fa reads.raw (timing and COMMAND lines stripped)
  rep_<tag>.reorder.json           the stderr of the same reads with the orphan moved to the front, and to the end
  rep_two_seq.fa, rep_dup_ref.fa, rep_zero_twice.fa, rep_thrice.fa, rep_errors.json    references that -R refuses or just accepts, with its FATAL ERROR lines

Table bits 20: the smallest modsetCreate takes (modset.c:17)."""
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

REF = os.environ.get("MODGPU_REFERENCE_SRC", "/root/reference")
MU = os.path.join(ROOT, "oracle", "_ref", "modutils_ref")
assert os.path.exists(MU) and os.path.exists(os.path.join(REF, "modrep.c")), "needs oracle/_ref and the reference's sources"

TAGS = {"k19d8": (19, 8, 5150), "k16d4": (16, 4, 5151)}      # k, w, seed of the genome
BITS = 20


def strip_noise(text):
    """drop the getrusage lines (utils.c:187-193) and the COMMAND echo (modrep.c:568-570)"""
    return "".join(l + "\n" for l in text.splitlines() if not l.startswith("user\t") and "resources used" not in l and not l.startswith("COMMAND "))


def run(cmd, cwd, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    assert (r.returncode == 0) == ok, (cmd, r.returncode, r.stderr[-2000:])
    return r.stdout, r.stderr


def rc(s):
    return (3 - s[::-1]).astype(np.uint8)


def make_reads(g, k, w):
    """(names, reads): see the module's text and the assertions in gen ()"""
    cat = np.concatenate
    seg = 50 * w                                                       # ~50 reference hits
    reads = [
        ("tandem", cat([g[40000:41200], g[40000:41200], g[41200:42500]])),      # every mod of the first part twice: dups
        ("a1", g[0:3000]), ("a2_rc", rc(g[1500:4500])), ("a3", g[3000:6000]),     # depth 2 at the most
        ("junk", synth.iid_bases(2000, 777)),                          # n 0
        ("few_hits", g[50000:50000 + 60 * w]),                         # fewer than 100 reference hits
        ("chimera", cat([g[56000:56000 + seg], rc(g[56000 + seg:56000 + 2 * seg]), g[56000 + 2 * seg:56000 + 3 * seg], rc(g[56000 + 3 * seg:56000 + 4 * seg]),
                         g[56000 + 4 * seg:56000 + 5 * seg], rc(g[56000 + 5 * seg:56000 + 6 * seg])])),      # both strands inside the first 100
        ("empty", g[0:0]),
        ("shorter_than_k", g[100:100 + k - 3]),
        ("fwd_then_rev", cat([g[45000:45000 + k + 5 * w], rc(g[46000:48000])])),      # a few forward hits, then reverse ones: good, flipped, seqF > 0
        ("orphan", g[52000:55000]),                                    # good against the reference, nothing of it in the second set
        ("b1", g[20000:24000]), ("b2_rc", rc(g[20500:24500])), ("b3", g[21000:25000]), ("b4_rc", rc(g[21500:25500])), ("b5", g[22000:26000]),      # depth 5
        ("c1", g[30000:33000]), ("c2_rc", rc(g[30500:33500])), ("c3", g[31000:34000]),      # depth 3
    ]
    return [n for n, _ in reads], [s for _, s in reads]


def summary(err):
    m = re.search(r"^read (\d+) reads, (\d+) bad, (\d+) good: mods total (\d+) good (\d+) dup (\d+) avdup ([0-9.]+)$", err, re.M)
    q = re.search(r"^minimum max for a read is (\d+)$", err, re.M)
    assert m and q, err
    return [int(x) for x in m.groups()[:6]], int(q.group(1))


def gunzip_to(src, dst):
    open(dst, "wb").write(gzip.open(src).read())


def gen(tag, k, w, seed, modrep, tmp):
    stem = "rep_%s" % tag
    g = synth.iid_bases(60000, seed)
    names, reads = make_reads(g, k, w)
    orphan = names.index("orphan")
    fasta.write_fasta(os.path.join(HERE, stem + "_ref.fa"), ["ref"], [g])
    fasta.write_fasta(os.path.join(HERE, stem + "_reads.fa"), names, reads)
    keep = [i for i in range(len(names)) if i != orphan]
    fasta.write_fasta(os.path.join(tmp, "src.fa"), [names[i] for i in keep] + ["junk_tail"], [reads[i] for i in keep] + [synth.iid_bases(1500, 999)])
    run([MU, "-c", str(BITS), str(k), str(w), "17", "-a", stem + "_ref.fa", "-w", stem + "_ref.mod"], HERE)
    run([MU, "-c", str(BITS), str(k), str(w), "17", "-a", os.path.join(tmp, "src.fa"), "-w", stem + "_reads.mod"], HERE)
    gunzip_to(os.path.join(HERE, stem + "_ref.mod"), os.path.join(tmp, "ref.raw"))
    gunzip_to(os.path.join(HERE, stem + "_reads.mod"), os.path.join(tmp, "reads.raw"))

    def rep(reads_fa):
        out, err = run([modrep, "-R", os.path.join(HERE, stem + "_ref.fa"), "ref.raw", "-s3", reads_fa, "reads.raw"], tmp)
        return strip_noise(out), strip_noise(err)
    out, err = rep(os.path.join(HERE, stem + "_reads.fa"))
    open(os.path.join(HERE, stem + ".stdout.txt"), "w").write(out)
    open(os.path.join(HERE, stem + ".stderr.txt"), "w").write(err)

    # ---- the fixture holds what it is for, by the reference's own output ----
    assert re.search(r"^found (\d+) of \1 locations in ref length 60000$", err, re.M), err
    bad = {int(m.group(1)): [int(x) for x in m.groups()[1:]] for m in re.finditer(r"^BADREAD +(\d+) len +(\d+) n (\d+) F +(\d+) R +(\d+)$", out, re.M)}
    no = {n: i + 1 for i, n in enumerate(names)}
    assert sorted(bad) == sorted(no[n] for n in ("junk", "few_hits", "chimera", "empty", "shorter_than_k")), bad
    assert bad[no["junk"]][1] == 0 and 0 < bad[no["few_hits"]][1] < 100 and bad[no["empty"]][:2] == [0, 0] and bad[no["shorter_than_k"]][1] == 0
    assert bad[no["chimera"]][1] == 100 and bad[no["chimera"]][2] > 10 and bad[no["chimera"]][3] > 10
    counts, min_max = summary(err)
    assert counts[0] == len(names) and counts[1] == 5 and counts[2] == len(names) - 5
    assert counts[4] + counts[5] == counts[3] and counts[5] > 0, counts       # good + dup == max: entry 0 counted, entry max not
    assert min_max > 1, min_max
    moved = {}
    for where, order in (("orphan_first", [orphan] + keep), ("orphan_last", keep + [orphan])):
        fasta.write_fasta(os.path.join(tmp, where + ".fa"), [names[i] for i in order], [reads[i] for i in order])
        o2, e2 = rep(where + ".fa")
        moved[where] = {"order": order, "stdout": o2, "stderr": e2}
    assert 0 < summary(moved["orphan_first"]["stderr"])[1] < min_max      # the fold starts again at the orphan: without it in the way the shallow reads count
    assert summary(moved["orphan_last"]["stderr"])[1] == 0
    json.dump(moved, open(os.path.join(HERE, stem + ".reorder.json"), "w"), indent=1)
    print(stem, counts, "minimum max", min_max, "orphan first", summary(moved["orphan_first"]["stderr"])[1],
          "| sizes", {e: os.path.getsize(os.path.join(HERE, stem + e)) for e in ("_ref.fa", "_ref.mod", "_reads.fa", "_reads.mod", ".stdout.txt", ".stderr.txt", ".reorder.json")})


def gen_errors(modrep, tmp):
    """references against rep_k19d8_ref.mod: two records; a mod-bearing stretch repeated; a mod at position 0 twice (accepted); the same thrice"""
    k, w, seed = TAGS["k19d8"]
    g = synth.iid_bases(60000, seed)
    gunzip_to(os.path.join(HERE, "rep_k19d8_ref.mod"), os.path.join(tmp, "ref.raw"))
    out, _ = run([MU, "-r", "rep_k19d8_ref.mod", "-P", "rep_k19d8_ref.fa"], HERE)
    locs = [int(l.split()[0]) for l in out.splitlines() if l.startswith("  ")]
    p0 = locs[len(locs) // 2]                                           # a modimizer's position: g[p0 : p0 + k] is in the set
    head = g[p0:p0 + 300]                                               # a sequence that starts with a mod
    cases = {
        "rep_two_seq.fa": (["one", "two"], [g[:3000], g[3000:6000]]),
        "rep_dup_ref.fa": (["dup"], [np.concatenate([g[:5000], g[2000:3000]])]),
        "rep_zero_twice.fa": (["zero_twice"], [np.concatenate([head[:k], synth.iid_bases(40, 4242), head[:k]])]),
        "rep_thrice.fa": (["thrice"], [np.concatenate([head[:k], synth.iid_bases(40, 4242), head[:k], synth.iid_bases(40, 4243), head[:k]])]),
    }
    rec = {}
    for name, (nn, ss) in cases.items():
        fasta.write_fasta(os.path.join(HERE, name), nn, ss)
        r = subprocess.run([modrep, "-R", os.path.join(HERE, name), "ref.raw"], capture_output=True, text=True, cwd=tmp)
        err = strip_noise(r.stderr)
        fatal = [l for l in err.splitlines() if l.startswith("FATAL ERROR")]
        rec[name] = {"fatal": fatal[0] if fatal else None, "stderr": err}
    assert rec["rep_two_seq.fa"]["fatal"] == "FATAL ERROR: multiple sequences in ref file - only one allowed", rec
    assert re.match(r"FATAL ERROR: duplicate mod entry at position \d+ in ref$", rec["rep_dup_ref.fa"]["fatal"]), rec
    assert rec["rep_zero_twice.fa"]["fatal"] is None and rec["rep_zero_twice.fa"]["stderr"].startswith("found 2 of "), rec      # position 0 does not protect its entry
    assert re.match(r"FATAL ERROR: duplicate mod entry at position \d+ in ref$", rec["rep_thrice.fa"]["fatal"]), rec
    json.dump(rec, open(os.path.join(HERE, "rep_errors.json"), "w"), indent=1)
    print("errors", {n: v["fatal"] for n, v in rec.items()})


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="modrep_golden_")
    try:
        modrep = os.path.join(tmp, "modrep_ref")
        lib_src = [os.path.join(REF, f) for f in ("seqhash.c", "modset.c", "utils.c", "array.c", "hash.c", "dict.c")]
        subprocess.check_call(["gcc", "-O2", "-w", "-no-pie", "-o", modrep, os.path.join(REF, "modrep.c"), os.path.join(REF, "seqio.c")] + lib_src
                              + ["-lz", "-l:libbsd.so.0", "-lm"])
        for tag, (k, w, seed) in TAGS.items():
            gen(tag, k, w, seed, modrep, tmp)
        gen_errors(modrep, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
