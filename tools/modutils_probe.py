"""dev probe: what the summary and -x cost, against what they replace.
  summary   mgModsetSummaryDevice against modsetSummary on config 2's set (10 Gbp of synthetic long reads, k = 21, w = 64, table bits 30:
            1.03e8 entries).  modsetSummary syncs value[] / depth[] and walks them on the host; its first call after a build pays the
            sync, a second one only the host loop.  Both must print the same bytes.
  -s        mgModsetSetCopy on the same set.
  -x        mgAddSequenceFile10x against mgAddSequenceFile on one plain FASTQ file of 150-base reads (the sets differ: -x drops 23 bases
            of every other read).
usage: python tools/modutils_probe.py [out.json] [fastq_reads]   (GPU box; prints the JSON of every figure)"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import modimizer_amd as mg  # noqa: E402
from report_probe import device_set  # noqa: E402


def clock(f, *a):
    t = time.perf_counter()
    r = f(*a)
    return r, round((time.perf_counter() - t) * 1e3, 3)


def write_fastq(path, n_reads, seed=7):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    genome = lut[rng.integers(0, 4, 5_000_000)]
    qual = b"I" * 150
    with open(path, "wb") as f:
        for c in range(0, n_reads, 100000):
            at = rng.integers(0, len(genome) - 150, min(100000, n_reads - c))
            f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (c + i, genome[a:a + 150].tobytes(), qual) for i, a in enumerate(at)))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
    L = mg.lib()
    mg.check(L.mgSetDevice(0))
    res = {"set": "config 2: 10 Gbp synthetic long reads, k=21 w=64 table bits 30"}
    tmp = tempfile.mkdtemp()
    ms = device_set(L, 10_000_000_000, 333_333_333, 1000, 777)
    res["entries"] = int(ms.contents.max)
    dev, res["summary_device_ms_first"] = clock(mg.summary_device, ms, os.path.join(tmp, "d.txt"))
    res["summary_device_ms"] = [clock(mg.summary_device, ms, os.path.join(tmp, "d.txt"))[1] for _ in range(3)]
    _, res["set_copy_device_ms_first"] = clock(mg.set_copy, ms, 5, 20, 60)
    res["set_copy_device_ms"] = [clock(mg.set_copy, ms, 5, 20, 60)[1] for _ in range(2)]
    # info[] has been written now (-s brought all of it back): the summary uploads every page of it, no longer a sparse array
    res["summary_device_ms_info_written"] = [clock(mg.summary_device, ms, os.path.join(tmp, "d.txt"))[1] for _ in range(3)]
    dev2 = mg.summary_device(ms, os.path.join(tmp, "d.txt"))

    def host_summary():
        with mg.CFile(os.path.join(tmp, "h.txt"), "w") as f:
            L.modsetSummary(ms, f)
        return open(os.path.join(tmp, "h.txt")).read()
    host, res["modsetSummary_ms_with_sync"] = clock(host_summary)
    res["modsetSummary_ms_synced"] = [clock(host_summary)[1] for _ in range(2)]
    res["same_bytes"] = bool(host == dev2) and dev.splitlines()[:2] == host.splitlines()[:2]
    L.modsetDestroy(ms)

    fq = os.path.join(tmp, "reads.fq")
    write_fastq(fq, n_reads)
    res["fastq"] = {"reads": n_reads, "bases": 150 * n_reads, "bytes": os.path.getsize(fq)}
    for name, call in (("mgAddSequenceFile", lambda m, f: L.mgAddSequenceFile(m, fq.encode(), f)),
                       ("mgAddSequenceFile10x", lambda m, f: L.mgAddSequenceFile10x(m, fq.encode(), f))):
        times = []
        for _ in range(3):
            m = mg.modsetCreate(mg.seqhashCreate(21, 64, 17), 26)
            with mg.CFile(os.path.join(tmp, "a.txt"), "w") as f:
                rc, ms_ = clock(call, m, f)
            assert rc == 0, L.mgLastError()
            times.append(ms_)
            L.modsetDestroy(m)
        res[name + "_ms"] = times
        res[name + "_line"] = open(os.path.join(tmp, "a.txt")).read().strip()
    d = (C.c_uint64 * 4)(); L.mgAdd10xDiag(d)
    res["add10x_diag"] = [int(x) for x in d]
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
