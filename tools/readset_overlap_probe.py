"""dev probe: modasm -b -c (mgReadsetMarkBadReads, mgReadsetMarkContained) on a synthetic read set -- by default about 2 x 10^4 reads of 10 kb
at 20x over an iid genome, the source .mod made by modutils -s 1 2 3 -- on the device, by the library's host loops and by the reference
program (oracle/_ref/modasm_ref -r stem -b -c, less what -r alone takes).  One warm-up, then repeated runs, each on a fresh load of the
set; prints the runs, their median and spread, the counters of mgReadsetOverlapsDiag and the kernel split (mgProfile*), and one JSON line.
(tools/overlap_probe.py is an older probe about two pipelines on two streams; this one is about the reads' overlaps.)
usage: python tools/readset_overlap_probe.py [--reads N] [--len L] [--cov C] [--k K] [--w W] [--runs R] [--no-ref] [--no-host] [out.json]"""
import argparse
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import modimizer_amd as mg  # noqa: E402
from modimizer_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def kernel_ms(L):
    out = {}
    for i in range(L.mgProfileKernels()):
        nm, ms, n = C.c_char_p(), C.c_double(), C.c_uint64()
        L.mgProfileGet(i, C.byref(nm), C.byref(ms), C.byref(n))
        if n.value:
            out[nm.value.decode()] = (round(ms.value, 3), n.value)
    return out


def write_fasta(path, names, seqs, width=0):
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + lut[s].tobytes() + b"\n")


def make_files(d, a):
    rng = np.random.default_rng(2024)
    G = a.reads * a.len // a.cov
    g = synth.iid_bases(G, 4242)
    write_fasta(os.path.join(d, "src.fa"), ["chr"], [g])
    starts = rng.integers(0, G - a.len, a.reads)
    seqs = []
    for i, s in enumerate(starts):
        r = g[s:s + a.len].copy()
        m = rng.random(a.len) < 0.02
        r[m] = (r[m] + 1 + rng.integers(0, 3, int(m.sum()))) & 3
        seqs.append((3 - r[::-1]).astype(np.uint8) if i & 1 else r)
    write_fasta(os.path.join(d, "reads.fa"), ["r%d" % i for i in range(a.reads)], seqs)
    bits = max(20, int(np.ceil(np.log2(2.0 * G / a.w))) + 2)      # (a set holds a quarter of its table's slots)
    subprocess.check_call([os.path.join(REF, "modutils_ref"), "-c", str(bits), str(a.k), str(a.w), "17", "-a", "src.fa", "-s", "1", "2", "3", "-w", "src.mod"],
                          cwd=d, stdout=subprocess.DEVNULL)
    raw = open(os.path.join(d, "src.mod"), "rb").read()
    if raw[:2] == b"\x1f\x8b":                                     # the reference program writes gzip; modsetRead takes the plain bytes
        open(os.path.join(d, "src.mod"), "wb").write(gzip.decompress(raw))
    L = mg.lib()
    with mg.CFile(os.path.join(d, "src.mod"), "r") as f:
        ms = L.modsetRead(f)
    rs = L.mgReadsetCreate(ms)
    assert L.mgReadsetFileRead(rs, os.path.join(d, "reads.fa").encode()) == 0
    L.mgReadsetWrite(rs, os.path.join(d, "set").encode())
    out = dict(genome=G, reads=rs.contents.nReads, hits=int(rs.contents.totHit), mods=int(ms.contents.max))
    L.mgReadsetDestroy(rs)
    return out


def one_run(d, host):
    """(-b seconds, -c seconds, diag of -b, diag of -c, the lines) on a fresh load"""
    L = mg.lib()
    rs = L.mgReadsetLoad(os.path.join(d, "set").encode())
    with mg.CFile(os.path.join(d, "lines.txt"), "w") as f:
        t0 = time.perf_counter(); pb = mg.readset_mark_bad_reads(rs, f); t1 = time.perf_counter(); db = mg.readset_overlaps_diag()
        pc = mg.readset_mark_contained(rs, f); t2 = time.perf_counter(); dc = mg.readset_overlaps_diag()
    assert pb == pc == host, (pb, pc, host)
    L.mgReadsetDestroy(rs)
    return t1 - t0, t2 - t1, db, dc, open(os.path.join(d, "lines.txt")).read()


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4), runs=len(v))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reads", type=int, default=20000); p.add_argument("--len", type=int, default=10000); p.add_argument("--cov", type=int, default=20)
    p.add_argument("--k", type=int, default=19); p.add_argument("--w", type=int, default=31); p.add_argument("--runs", type=int, default=3)
    p.add_argument("--no-ref", action="store_true"); p.add_argument("--no-host", action="store_true"); p.add_argument("out", nargs="?")
    a = p.parse_args()
    L = mg.lib(); mg.check(L.mgSetDevice(0))
    res = {}
    with tempfile.TemporaryDirectory() as d:
        res["set"] = make_files(d, a)
        print("set:", res["set"], flush=True)
        one_run(d, 0)                                                            # warm-up: code objects, the transfer threads, the file cache
        L.mgProfileEnable(1); L.mgProfileReset()
        runs = [one_run(d, 0) for _ in range(a.runs)]
        res["kernels_ms_over_runs"] = kernel_ms(L); L.mgProfileEnable(0)
        res["device"] = dict(b=spread([r[0] for r in runs]), c=spread([r[1] for r in runs]), diag_b=runs[0][2], diag_c=runs[0][3])
        lines = runs[0][4]
        print("device:", res["device"], flush=True)
        if not a.no_host:
            os.environ["MODGPU_READSET_HOST"] = "1"; L.mgReloadKnobs()
            hruns = [one_run(d, 1) for _ in range(max(1, a.runs - 1))]
            del os.environ["MODGPU_READSET_HOST"]; L.mgReloadKnobs()
            assert all(r[4] == lines for r in hruns), "host loops and device print different lines"
            res["host_loops"] = dict(b=spread([r[0] for r in hruns]), c=spread([r[1] for r in hruns]))
            print("host loops:", res["host_loops"], flush=True)
        if not a.no_ref:
            def ref(cmd):
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(REF, "modasm_ref"), "-r", "set"] + cmd, cwd=d, capture_output=True, text=True)
                if r.returncode:
                    raise RuntimeError(r.stderr[-500:])
                return time.perf_counter() - t0, r.stdout
            try:
                load = [ref([])[0] for _ in range(2)]
                both = [ref(["-b", "-c"]) for _ in range(max(1, a.runs - 1))]
                ref_lines = "".join(l + "\n" for l in both[0][1].splitlines() if l.startswith(("MB", "MC")))
                res["reference"] = dict(load=spread(load), load_b_c=spread([r[0] for r in both]), same_lines=ref_lines == lines)
            except RuntimeError as e:
                res["reference"] = dict(error=str(e))
            print("reference:", res["reference"], flush=True)
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
