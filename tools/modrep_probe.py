"""dev probe: modrep -R / -s3 / -s1 (mgRepRefCreate, mgRepAnalyze3File, mgRepAnalyze1File) at one stated size -- a 5 Mbp iid reference at k 25 w 8, 10 000 reads of
10 kb from both strands with 1 % substitutions (100 Mbp), the second set made of the reads and a junk tail (so entry max is in no read, which -s1 needs) -- with the host's part (reading the .mod, parsing
the FASTA) timed by itself, and the reference program on the same files where a build of it is at hand (oracle/ builds none).
usage: python tools/modrep_probe.py [--reads N] [--modrep PATH_TO_REFERENCE_MODREP] [out_dir]   (GPU box; prints the JSON of every figure)"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import modimizer_amd as mg  # noqa: E402
from modimizer_amd import synth  # noqa: E402

K, W, BITS, GENOME, READ_LEN = 25, 8, 24, 5000000, 10000
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def write_fasta(path, names, seqs):
    """one line per sequence (the library's own writer formats base by base in Python)"""
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + LETTERS[s].tobytes() + b"\n")


def make_set(path, seqs):
    """the set of `seqs` (k, w, seed 17) as a PLAIN .mod file: the reference's modrep opens it with fopen"""
    L = mg.lib()
    ms = mg.modsetCreate(mg.seqhashCreate(K, W, 17), BITS)
    for i in range(0, len(seqs), 2000):
        chunk = seqs[i:i + 2000]
        offs = np.zeros(len(chunk) + 1, np.int64); offs[1:] = np.cumsum([len(s) for s in chunk])
        mg.add_sequence_batch(ms, np.concatenate(chunk), offs)
    mg.check(L.modsetSyncToHost(ms, 1))
    with mg.CFile(path, "w") as f:
        L.modsetWrite(ms, f)
    n = ms.contents.max
    L.modsetDestroy(ms)
    return n


def timed(fn):
    t = time.perf_counter(); r = fn(); return r, time.perf_counter() - t


def main():
    args = sys.argv[1:]
    n_reads, modrep = 10000, None
    while args and args[0].startswith("--"):
        if args[0] == "--reads":
            n_reads = int(args[1])
        elif args[0] == "--modrep":
            modrep = args[1]
        args = args[2:]
    out_dir = args[0] if args else tempfile.mkdtemp(prefix="modrep_probe_")
    os.makedirs(out_dir, exist_ok=True)
    L = mg.lib()
    g = synth.iid_bases(GENOME, 4711)
    rng = np.random.default_rng(5)
    starts = rng.integers(0, GENOME - READ_LEN, n_reads)
    reads = []
    for j, a in enumerate(starts):
        s = g[a:a + READ_LEN].copy()
        m = rng.random(READ_LEN) < 0.01
        s[m] = (s[m] + 1 + rng.integers(0, 3, int(m.sum()))) & 3
        reads.append((3 - s[::-1]).astype(np.uint8) if j & 1 else s)
    ref_fa, ref_mod, reads_fa, reads_mod = (os.path.join(out_dir, n) for n in ("ref.fa", "ref.mod", "reads.fa", "reads.mod"))
    write_fasta(ref_fa, ["ref"], [g]); write_fasta(reads_fa, ["r%d" % j for j in range(n_reads)], reads)
    fig = {"k": K, "w": W, "reference_bases": GENOME, "reads": n_reads, "read_bases": n_reads * READ_LEN,
           "ref_set_entries": make_set(ref_mod, [g]), "second_set_entries": make_set(reads_mod, reads + [synth.iid_bases(1500, 999)])}

    def whole(tag):
        ref, fig["R_s_" + tag] = timed(lambda: mg.rep_ref_create(ref_fa, ref_mod, os.path.join(out_dir, "R.err")))
        res, fig["s3_s_" + tag] = timed(lambda: mg.rep_analyze3_file(ref, reads_fa, reads_mod, os.path.join(out_dir, "s3.out"), os.path.join(out_dir, "s3.err")))
        res1, fig["s1_s_" + tag] = timed(lambda: mg.rep_analyze1_file(ref, reads_fa, reads_mod, os.path.join(out_dir, "s1.out"), os.path.join(out_dir, "s1.err")))
        fig["s1_diag"] = mg.rep1_diag()
        fig["s1_reads_kept"], fig["s1_mod_lines"] = res1["readsAfter"], int((res1["modN"][:-1] != 0).sum())
        L.mgRepRefDestroy(ref)
        return res
    whole("first"); res = whole("second")
    fig.update(good=res["nGood"], bad=res["nBad"], hits=int(res["hitStart"][-1]), dup=res["nDup"], min_max=res["minMax"])

    def host_parse():
        r = L.mgSeqOpen(reads_fa.encode()); b = mg.MgSeqBatch()
        while L.mgSeqNextBatch(r, 128000000, C.byref(b)) > 0:
            L.mgSeqBatchFree(C.byref(b))
        L.mgSeqClose(r)

    def host_mod():
        f = L.mgFzOpen(reads_mod.encode(), b"r"); ms = L.modsetRead(f); mg._libc.fclose(f); L.modsetDestroy(ms)
    fig["host_parse_reads_s"] = timed(host_parse)[1]
    fig["host_read_second_set_s"] = timed(host_mod)[1]
    if modrep and os.path.exists(modrep):
        r, fig["reference_program_s"] = timed(lambda: subprocess.run([modrep, "-R", ref_fa, ref_mod, "-s3", reads_fa, reads_mod], capture_output=True, text=True))
        ours = open(os.path.join(out_dir, "R.err")).read() + open(os.path.join(out_dir, "s3.err")).read()
        theirs = "".join(l + "\n" for l in r.stderr.splitlines() if l.startswith(("found ", "read ", "minimum ")))
        fig["same_lines_as_reference_program"] = (ours == theirs and r.stdout.count("BADREAD") == open(os.path.join(out_dir, "s3.out")).read().count("BADREAD"))
    print(json.dumps(fig, indent=1))
    if not args:
        shutil.rmtree(out_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
