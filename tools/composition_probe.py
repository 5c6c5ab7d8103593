#!/usr/bin/env python3
"""dev probe: mgCompositionFile (composition -b -q -l on the device) at size: a synthetic FASTA file of 10 kb reads and a FASTQ file of 150 b
reads with skewed qualities, a few GB each, written into tmpfs; GB/s of text with all three flags, after a warm-up call, median and spread
of the repeats.  Beside it, on the same files in the same run, the device text parser handing its batches to the test hook's sink
(mgTextParseFileDevice: it moves the same bytes over the link, reads them three times and writes the bases -- and the hook then copies
them to the host, so it is an upper bound on the parser's own time).  MODGPU_LIB chooses a variant build of the library
(tools/build_variant.sh hist0 -DCP_HIST_MODE=0: the histogram shapes of DESIGN_EXPERIMENTS.md).
usage: composition_probe.py [--gb 2] [--repeats 5] [--dir /dev/shm] [--skip-parser] [--skew]     (--skew: one base, one quality)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import modimizer_amd as mg      # noqa: E402


def write_fasta(path, total, rng, skew):
    """reads of 10 kb, lines of 80: one block of 64 MiB repeated"""
    recs = []
    for i in range(6400):
        s = np.full(10000, ord("A"), np.uint8) if skew else rng.choice(np.frombuffer(b"ACGT", np.uint8), 10000)
        lines = np.concatenate([s.reshape(125, 80), np.full((125, 1), 10, np.uint8)], axis=1).reshape(-1)
        recs.append(b">read%06d\n" % i + lines.tobytes())
    return repeat(path, b"".join(recs), total)


def write_fastq(path, total, rng, skew):
    """reads of 150 b; qualities almost one symbol (92 % '~'), the rest spread"""
    recs = []
    for i in range(100000):
        s = np.full(150, ord("A"), np.uint8) if skew else rng.choice(np.frombuffer(b"ACGT", np.uint8), 150)
        q = np.full(150, ord("~"), np.uint8)
        if not skew:
            low = rng.random(150) < 0.08
            q[low] = rng.integers(33, 127, int(low.sum()))
        recs.append(b"@read%06d\n" % i + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return repeat(path, b"".join(recs), total)


def repeat(path, block, total):
    n = max(1, total // len(block))
    with open(path, "wb") as f:
        for _ in range(n):
            f.write(block)
    return n * len(block)


def timed(fn, repeats):
    fn()                                                     # warm-up: buffers, page cache
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--skip-parser", action="store_true")
    ap.add_argument("--skew", action="store_true")
    a = ap.parse_args()
    L = mg.lib()
    rng = np.random.default_rng(7)
    out = {"lib": os.environ.get("MODGPU_LIB", "tree"), "skew": a.skew}
    for kind, write in (("fasta", write_fasta), ("fastq", write_fastq)):
        path = os.path.join(a.dir, "composition_probe_%d.%s" % (os.getpid(), kind[-1] == "a" and "fa" or "fq"))
        try:
            size = write(path, int(a.gb * (1 << 30)), rng, a.skew)
            res = mg.MgComposition()

            def comp():
                rc = L.mgCompositionFile(path.encode(), 7, None, None, C.byref(res))
                assert rc == 0, L.mgLastError()
                L.mgCompositionFree(C.byref(res))
            t = timed(comp, a.repeats)
            d = mg.composition_diag()
            row = {"bytes": size, "records": int(res.nSeq), "composition_GBps": round(size / statistics.median(t) / 1e9, 2),
                   "composition_GBps_min_max": [round(size / max(t) / 1e9, 2), round(size / min(t) / 1e9, 2)], "windows": d["windows"], "launches": d["launches"]}
            if not a.skip_parser:
                def parse():
                    b, o, n = C.c_void_p(), C.c_void_p(), C.c_int64()
                    rc = L.mgTextParseFileDevice(path.encode(), C.byref(b), C.byref(o), C.byref(n))
                    assert rc == 0, (rc, L.mgLastError())
                    mg._libc.free(b); mg._libc.free(o)
                tp = timed(parse, max(2, a.repeats // 2))
                row["parser_hook_GBps"] = round(size / statistics.median(tp) / 1e9, 2)
            out[kind] = row
        finally:
            if os.path.exists(path):
                os.unlink(path)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
