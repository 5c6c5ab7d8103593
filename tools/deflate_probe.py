#!/usr/bin/env python3
"""BGZF deflate on the device, measured: on the FASTQ and the FASTA text of tools/inflate_probe.py, in tmpfs,

  - the kernel alone (mgDeflateBlocksDevice on the whole text's 65280-byte blocks, text and members resident on the device): GB/s of text,
    against zlib level 1 on 16 host threads over the same blocks;
  - the compressed size against zlib levels 1 and 6 over the same blocks;
  - mgSeqConvertFileBgzf to .fa.gz against mgSeqConvertFile to .fa.gz (host zlib behind the link: what the commit before had) and to a plain file;
  - mgBgzfDeflateFile of the plain text;
  - mgDeflateDiag of each call.

  python tools/deflate_probe.py [--gib 1.0] [--dir /dev/shm] [--json out.json]
  MODGPU_SEED_TIMING=1 python tools/deflate_probe.py ...       the conversion's per-stage times on stderr

Times are host clocks around calls that end in a device synchronise; every figure is the best of --reps runs after one warm-up."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib
from multiprocessing.pool import ThreadPool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import modimizer_amd as mg  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inflate_probe import best, fasta_text, fastq_text  # noqa: E402  (the same two texts)

BLOCK = 65280


def kernel_rate(text, reps):
    n = -(-len(text) // BLOCK)
    tab = (mg.MgGzBlock * n)(*[mg.MgGzBlock(i * BLOCK, min(BLOCK, len(text) - i * BLOCK), 0) for i in range(n)])
    d_text, d_out = mg.DeviceBuffer.from_numpy(np.frombuffer(text, np.uint8)), mg.DeviceBuffer(65536 * n)
    off = (C.c_uint64 * (n + 1))()

    def run():
        mg.check(mg.lib().mgDeflateBlocksDevice(d_text.ptr, len(text), tab, n, d_out.ptr, 65536 * n, off, None))
    t, _ = best(run, reps)
    packed = d_out.to_numpy(np.uint8, int(off[n])).tobytes()
    d_text.free(); d_out.free()
    kinds = [0, 0, 0]
    for i in range(0, n, max(1, n // 64)):                # what the blocks became, on a sample
        kinds[mg.deflate_block_host(text[i * BLOCK:(i + 1) * BLOCK])[1]["kind"]] += 1
    return dict(seconds=t, text_gb_s=len(text) / t / 1e9, blocks=n, payload_bytes=int(off[n]) - 26 * n, file_bytes=int(off[n]) + 28, diag=mg.deflate_diag(),
                sampled_kinds=kinds), packed


def zlib_threads(text, level, threads, reps):
    view = memoryview(text)

    def one(rng):
        n = 0
        for i in range(rng[0], rng[1]):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            n += len(c.compress(view[i * BLOCK:(i + 1) * BLOCK])) + len(c.flush())
        return n
    blocks = -(-len(text) // BLOCK)
    step = max(1, blocks // (threads * 8))
    ranges = [(i, min(blocks, i + step)) for i in range(0, blocks, step)]
    with ThreadPool(threads) as pool:
        t, n = best(lambda: sum(pool.map(one, ranges)), reps)
    return dict(seconds=t, text_gb_s=len(text) / t / 1e9, payload_bytes=n, threads=threads, level=level)


def file_calls(plain, reps):
    out = {}
    new = hasattr(mg.lib(), "mgSeqConvertFileBgzf")
    cases = [("gz_host_zlib", lambda dst: mg.seq_convert_file(plain, dst, mg.SEQ_FASTA), ".fa.gz"), ("plain", lambda dst: mg.seq_convert_file(plain, dst, mg.SEQ_FASTA), ".fa")]
    if new:
        cases.insert(0, ("bgzf_device", lambda dst: mg.seqconvert_file_bgzf(plain, dst, mg.SEQ_FASTA), ".fa.gz"))
    for name, call, suffix in cases:
        dst = plain + ".out" + suffix
        t, r = best(lambda: call(dst), reps)
        out["seqconvert_" + name] = dict(seconds=t, n_seq=r[1]["nSeq"], out_bytes=os.path.getsize(dst), diag=mg.deflate_diag() if new else None)
        os.remove(dst)
    if new:
        dst = plain + ".gz"
        t, _ = best(lambda: mg.bgzf_deflate_file(plain, dst), reps)
        out["bgzip"] = dict(seconds=t, text_gb_s=os.path.getsize(plain) / t / 1e9, out_bytes=os.path.getsize(dst), diag=mg.deflate_diag())
        t, ok = best(lambda: mg.bgzf_inflate_file(dst, plain + ".back"), 1)
        out["bgzip_reads_back"] = bool(ok) and os.path.getsize(plain + ".back") == os.path.getsize(plain)
        os.remove(dst); os.remove(plain + ".back")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--calls-only", action="store_true", help="only the file calls (an older library: MODGPU_LIB)")
    a = ap.parse_args()
    result = dict(gib=a.gib, library="this tree" if not os.environ.get("MODGPU_LIB") else os.environ["MODGPU_LIB"])
    for kind, make, share in (("fastq", fastq_text, 1.0), ("fasta", fasta_text, 0.5)):
        plain = os.path.join(a.dir, "deflate_probe." + kind)
        text = make(int(a.gib * share * (1 << 30)))
        open(plain, "wb").write(text)
        r = dict(text_bytes=len(text))
        if not a.calls_only:
            r["kernel"], packed = kernel_rate(text, a.reps)
            head = zlib.decompressobj(31).decompress(packed[:1 << 16])
            assert head == text[:len(head)] and len(head) == BLOCK
            r["zlib_level_1_16_threads"] = zlib_threads(text, 1, 16, a.reps)
            r["zlib_level_6_16_threads"] = zlib_threads(text, 6, 16, 1)
            del packed
        del text
        r["calls"] = file_calls(plain, a.reps)
        os.remove(plain)
        result[kind] = r
        print(kind, json.dumps(r), flush=True)
    if a.json:
        json.dump(result, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
