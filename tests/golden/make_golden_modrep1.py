#!/usr/bin/env python3
"""Generate tests/golden/rep1_* by running the REFERENCE ITSELF, as make_golden_modrep.py does: oracle/_ref/modutils_ref for the second
set, and modrep, compiled here from the reference's modrep.c into a temporary directory, run, and deleted with the directory.  Only where
the reference's sources are.  The outputs are data: inputs and the reference's answers.  Re-run with:  python tests/golden/make_golden_modrep1.py

The reference is the existing rep_k19d8_ref.fa / _ref.mod (k 19, w 8; more than 2961 entries, which -s2's four indices need).

  rep1_reads.fa                 at most 40 reads of 3-6 kb from the 60 kb genome (see make_reads)
  rep1_reads.mod                the second set: the reads, then a junk tail that no read holds, so entry max is in no read
  rep1.stdout.txt / .stderr.txt modrep -R rep_k19d8_ref.fa ref.raw -s1 rep1_reads.fa reads.raw -s2 rep1_reads.fa reads.raw (timing and COMMAND lines stripped)
  rep1_max_reads.fa / .mod      a smaller file whose set has NO junk tail: its last read holds entry max
  rep1_max.note.txt             that the reference does not finish cleanly on it (modrep.c:288,343 index mods[ms->max]); no output is kept
"""
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
sys.path.insert(0, HERE)
from modimizer_amd import fasta, synth     # noqa: E402
from oracle import pyoracle                # noqa: E402
from make_golden_modrep import REF, MU, TAGS, BITS, strip_noise, run, rc, gunzip_to      # noqa: E402

K, W, SEED = TAGS["k19d8"]
BOUNDARY = (1, 961, 1951, 2961)


def make_reads(g, pos):
    """(names, reads).  pos[i]: the position of reference entry i in g.
      t*    31 reads of 4 kb that tile g[28000:39500] from a start every 250 bases, as a sequencing run tiles a genome: depth 16, between
            the 5 and the half of the good reads that cleanMods keeps.  The first mod of every read has a predecessor in the reads before it and
            none in its own: these are the mods that survive `no new info` (modrep.c:377), one a read.  The chain of the run removal (hits
            closer than k) starts at another hit in every read, so mods lose part of their count.  The outermost reads hold links that
            fewer than 5 reads share: they are dropped as reads with weak links.
            Ten segments of 300 bases, one every 1000: every second read that spans segment q lacks it (t*_d<kb>; reads of odd j + q): the last
            surviving mod before a gap has two `post` entries, the first behind it two `pre`, and which of the two arrives first changes from
            segment to segment.  t07 is t06 again: a BLOCK of 2.  Every third read is reverse-complemented.
      s2_*  reads joined from the neighbourhoods of two of -s2's four reference entries (1 / 961, 961 / 1951, 1951 / 2961, 2961 / 1): 3, 2, 1 and 2 of them
      few_hits   a bad read"""
    cat = np.concatenate
    reads = []
    for j in range(31):
        a = 28000 + 250 * (j - 1 if j == 7 else j)
        cuts = [c for q, c in enumerate(range(29000, 39000, 1000)) if (j + q) % 2 and a + 200 <= c and c + 300 + 200 <= a + 4000]
        s = cat([g[lo:hi] for lo, hi in zip([a] + [c + 300 for c in cuts], cuts + [a + 4000])])
        reads.append(("t%02d%s%s" % (j, "".join("_d%d" % (c // 1000) for c in cuts), "_rc" if j % 3 == 2 else ""), rc(s) if j % 3 == 2 else s))
    around = lambda i: g[max(0, pos[i] - 1500):pos[i] + 1500]
    for j, copies in enumerate((3, 2, 1, 2)):
        i0, i1 = BOUNDARY[j], BOUNDARY[(j + 1) % 4]
        for c in range(copies):
            reads.append(("s2_%d_%d_%d" % (i0, i1, c), cat([around(i0), around(i1)])))
    reads.append(("few_hits", g[50000:50000 + 60 * W]))
    assert len(reads) <= 40
    return [n for n, _ in reads], [s for _, s in reads]


def build_set(tmp, names, reads, out_mod, junk_tail):
    src = os.path.join(tmp, "src.fa")
    fasta.write_fasta(src, names + (["junk_tail"] if junk_tail else []), reads + ([synth.iid_bases(1500, 999)] if junk_tail else []))
    run([MU, "-c", str(BITS), str(K), str(W), "17", "-a", src, "-w", out_mod], HERE)


def gen(modrep, tmp):
    g = synth.iid_bases(60000, SEED)
    assert np.array_equal(fasta.read_fasta_list(os.path.join(HERE, "rep_k19d8_ref.fa"))[0], g)
    kmer, loc, _ = pyoracle.Hasher(K, W, 17).scan(g)
    assert len(np.unique(kmer)) == len(kmer) > BOUNDARY[3]                 # entry i is the genome's i-th modimizer, and the set has more than 2961
    pos = np.concatenate([[0], loc]).astype(int)
    names, reads = make_reads(g, pos)
    assert all(3000 <= len(s) <= 6000 for n, s in zip(names, reads) if n != "few_hits"), [(n, len(s)) for n, s in zip(names, reads)]
    fasta.write_fasta(os.path.join(HERE, "rep1_reads.fa"), names, reads)
    build_set(tmp, names, reads, "rep1_reads.mod", True)
    gunzip_to(os.path.join(HERE, "rep_k19d8_ref.mod"), os.path.join(tmp, "ref.raw"))
    gunzip_to(os.path.join(HERE, "rep1_reads.mod"), os.path.join(tmp, "reads.raw"))
    ref_fa, reads_fa = os.path.join(HERE, "rep_k19d8_ref.fa"), os.path.join(HERE, "rep1_reads.fa")
    out, err = run([modrep, "-R", ref_fa, "ref.raw", "-s1", reads_fa, "reads.raw", "-s2", reads_fa, "reads.raw"], tmp)
    err = re.sub(r"^(read \d+ reads, \d+ bad, \d+ good: )user\t[^\n]*$", r"\1", err, flags=re.M)      # timeUpdate writes on that line (modrep.c:351-352): a newline stands for it
    out, err = strip_noise(out), strip_noise(err)
    open(os.path.join(HERE, "rep1.stdout.txt"), "w").write(out)
    open(os.path.join(HERE, "rep1.stderr.txt"), "w").write(err)

    # ---- the fixture holds what it is for, by the reference's own output ----
    m = re.search(r"^found (\d+) of \1 locations in ref length 60000$", err, re.M)
    assert m and int(m.group(1)) == len(kmer), err
    m = re.search(r"^read (\d+) reads, (\d+) bad, (\d+) good: $", err, re.M)
    assert m and int(m.group(1)) == len(names) and int(m.group(3)) >= 10, err
    m = re.search(r"^reduced (\d+) reads to (\d+) reads$", err, re.M)
    assert m and 0 < int(m.group(2)) < int(m.group(1)), err
    nmod = [[int(x) for x in q.groups()] for q in re.finditer(r"^NMOD mod0 (\d+) modSmall (\d+) modBig (\d+) modGood (\d+)$", out, re.M)]
    assert len(nmod) == 5 and nmod[1][1] > 0, nmod                         # the second call's small mods: counts that the run removal took below 5
    mods = [l for l in out.splitlines() if l.startswith("MOD ")]
    assert len(mods) >= 20, len(mods)
    lists = [re.match(r"MOD (\d+) n \d+ pre \d+ \((.*?)\) post \d+ \((.*?)\)$", l).groups() for l in mods]
    assert any(len(p.split()) >= 2 for _, p, _ in lists) and any(len(q.split()) >= 2 for _, _, q in lists)
    blocks = [int(l.split()[1]) for l in out.splitlines() if l.startswith("BLOCK ")]
    assert blocks and max(blocks) > 1, blocks
    m = re.search(r"^n1 (\d+) n2 (\d+) n3 (\d+) n4 (\d+)$", out, re.M)
    n4 = [int(x) for x in m.groups()]
    assert min(n4) > 0 and len(set(n4)) > 1, n4
    # a move to the front: a printed list whose order is not the order of first arrival.  The surviving reads' hit lists are printed (READ
    # lines, in sorted order); their arrival order is the read's ordinal in the file
    rd = sorted(((int(l.split()[1]), [int(x) for x in l.split("mods")[1].split()]) for l in out.splitlines() if l.startswith("READ ")), key=lambda r: r[0])
    moved = 0
    for i, pre, post in lists:
        i = int(i)
        for text, side in ((pre, -1), (post, 1)):
            printed = [int(e.split(":")[0]) for e in text.split()]
            first = []
            for _, ks in rd:
                for j in range(len(ks)):
                    if ks[j] == i and 0 <= j + side < len(ks) and ks[j + side] not in first:
                        first.append(ks[j + side])
            assert sorted(first) == sorted(printed), (i, printed, first)
            moved += printed != first
    assert moved > 0
    # the run removal acts: the good reads' neighbouring modimizers lie closer than k somewhere (w < k: nearly everywhere)
    assert (np.diff(loc) < K).any()
    print("rep1", "nmod", nmod, "mods", len(mods), "blocks", blocks, "n4", n4, "moved lists", moved, err.splitlines()[-1],
          "| sizes", {e: os.path.getsize(os.path.join(HERE, "rep1" + e)) for e in ("_reads.fa", "_reads.mod", ".stdout.txt", ".stderr.txt")})


def gen_max(modrep, tmp):
    g = synth.iid_bases(60000, SEED)
    names = ["m%d" % j for j in range(14)]                                 # depth 6 of 14 reads: mods survive cleanMods, so the last read's hit on entry max has a neighbour
    reads = [g[20000 + 500 * j:23000 + 500 * j] for j in range(14)]
    fasta.write_fasta(os.path.join(HERE, "rep1_max_reads.fa"), names, reads)
    build_set(tmp, names, reads, "rep1_max_reads.mod", False)
    gunzip_to(os.path.join(HERE, "rep1_max_reads.mod"), os.path.join(tmp, "max.raw"))
    r = subprocess.run([modrep, "-R", os.path.join(HERE, "rep_k19d8_ref.fa"), "ref.raw", "-s1", os.path.join(HERE, "rep1_max_reads.fa"), "max.raw"],
                       capture_output=True, text=True, cwd=tmp)
    assert r.returncode != 0 and "total resources used" not in r.stderr, (r.returncode, r.stderr[-500:])
    open(os.path.join(HERE, "rep1_max.note.txt"), "w").write(
        "modrep -R rep_k19d8_ref.fa ref.raw -s1 rep1_max_reads.fa max.raw: the reference does not finish cleanly (exit status %d, no `total resources used` line)\n" % r.returncode)
    print("rep1_max", "exit status", r.returncode)


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="modrep1_golden_")
    try:
        modrep = os.path.join(tmp, "modrep_ref")
        lib_src = [os.path.join(REF, f) for f in ("seqhash.c", "modset.c", "utils.c", "array.c", "hash.c", "dict.c")]
        subprocess.check_call(["gcc", "-O2", "-w", "-no-pie", "-o", modrep, os.path.join(REF, "modrep.c"), os.path.join(REF, "seqio.c")] + lib_src
                              + ["-lz", "-l:libbsd.so.0", "-lm"])
        gen(modrep, tmp)
        gen_max(modrep, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
