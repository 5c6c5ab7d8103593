#!/usr/bin/env python3
"""dev probe: mgSeqConvertFile (seqconvert -fa / -fq and seqhoco on the device) at size: a synthetic FASTA file of 10 kb reads and a FASTQ
file of 150 b reads, a few GB each, written into tmpfs, and the five conversions fa -> fa, fa -> fq, fq -> fa, fq -> fq and hoco (of the
FASTA file), each written to a file in tmpfs that is deleted again.  Per conversion, after a warm-up call: GB/s of INPUT text over the whole
call (median and spread of the repeats) and, from the library's MODGPU_SEED_TIMING line of the median repeat, the stages as GB/s of input:
the first walk (judge: read + device, nothing written), the second walk (write), reading (both walks), the device-to-host copies, the
writer thread, and the kernels alone of either walk (between events on their stream).  The stages overlap, so they do not add up to the call.
usage: seqconvert_probe.py [--gb 2] [--repeats 3] [--dir /dev/shm]"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import modimizer_amd as mg      # noqa: E402


def repeat(path, block, total):
    n = max(1, total // len(block))
    with open(path, "wb") as f:
        for _ in range(n):
            f.write(block)
    return n * len(block)


def write_fasta(path, total, rng):
    """reads of 10 kb, lines of 80, mixed case: one block of 64 MiB repeated"""
    recs = []
    for i in range(6400):
        s = rng.choice(np.frombuffer(b"AACCGGTTacgt", np.uint8), 10000)
        lines = np.concatenate([s.reshape(125, 80), np.full((125, 1), 10, np.uint8)], axis=1).reshape(-1)
        recs.append(b">read%06d some words\n" % i + lines.tobytes())
    return repeat(path, b"".join(recs), total)


def write_fastq(path, total, rng):
    recs = []
    for i in range(100000):
        s = rng.choice(np.frombuffer(b"AACCGGTT", np.uint8), 150)
        q = rng.integers(33, 127, 150, dtype=np.uint8)
        recs.append(b"@read%06d some words\n" % i + s.tobytes() + b"\n+read%06d\n" % i + q.tobytes() + b"\n")
    return repeat(path, b"".join(recs), total)


class Stderr:
    """the C library's stderr of the block, as text"""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("latin-1")
        self.tmp.close()


STAGES = ("first_walk", "second_walk", "read", "d2h", "wait_for_block", "writer", "kernels_first_walk", "kernels_second_walk")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    out = {}
    files = {}
    dst = os.path.join(a.dir, "seqconvert_probe_%d.out" % os.getpid())
    try:
        for kind, write in (("fa", write_fasta), ("fq", write_fastq)):
            files[kind] = os.path.join(a.dir, "seqconvert_probe_%d.%s" % (os.getpid(), kind))
            files[kind + "_bytes"] = write(files[kind], int(a.gb * (1 << 30)), rng)
        for name, src, flags in (("fa_to_fa", "fa", mg.SEQ_FASTA), ("fa_to_fq", "fa", mg.SEQ_FASTQ), ("fq_to_fa", "fq", mg.SEQ_FASTA), ("fq_to_fq", "fq", mg.SEQ_FASTQ),
                                 ("hoco", "fa", mg.SEQ_HOCO)):
            size = files[src + "_bytes"]
            mg.seq_convert_file(files[src], dst, flags)        # warm-up: buffers, page cache
            runs = []
            with mg.knobs(SEED_TIMING=1):
                for _ in range(a.repeats):
                    with Stderr() as e:
                        t0 = time.perf_counter()
                        err, res = mg.seq_convert_file(files[src], dst, flags)
                        t = time.perf_counter() - t0
                    ms = [float(x) for x in re.findall(r"([0-9.]+) ms", [l for l in e.text.splitlines() if l.startswith("mgSeqConvert:")][-1])]
                    runs.append((t, ms, os.path.getsize(dst)))
            runs.sort(key=lambda r: r[0])
            t, ms, written = runs[len(runs) // 2]
            gbps = lambda sec: round(size / sec / 1e9, 2) if sec > 0 else None
            out[name] = {"in_bytes": size, "out_bytes": written, "records": res["nSeq"], "GBps": gbps(statistics.median(r[0] for r in runs)),
                         "GBps_min_max": [gbps(runs[-1][0]), gbps(runs[0][0])], "stages_GBps": {k: gbps(v / 1e3) for k, v in zip(STAGES, ms)},
                         "windows": mg.seq_convert_diag()["windows"], "launches": mg.seq_convert_diag()["launches"]}
    finally:
        for p in (files.get("fa"), files.get("fq"), dst):
            if p and os.path.exists(p):
                os.unlink(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
