#!/usr/bin/env python3
"""BGZF inflate on the device, measured: on a FASTQ and a FASTA text written as BGZF at level 6 into tmpfs,

  - the kernel alone (mgInflateMembersDevice on the whole file's members, compressed bytes and text resident on the device): GB/s of
    text with the CRC-32 and without it (MODGPU_INFLATE_NOCRC=1);
  - the same members inflated by zlib on 16 host threads;
  - mgCompositionFile and mgSeqConvertFile on the BGZF file with MODGPU_BGZF_HOST off and on, and on the plain file;
  - mgInflateDiag of each call.

  python tools/inflate_probe.py [--gib 1.0] [--dir /dev/shm] [--json out.json]
  MODGPU_LIB=<an older build> python tools/inflate_probe.py --calls-only --keep ...    the file calls alone, for the commit before

Times are host clocks around calls that end in a device synchronise; every figure is the best of --reps runs after one warm-up."""
import argparse
import json
import os
import sys
import time
import zlib
from multiprocessing.pool import ThreadPool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import modimizer_amd as mg  # noqa: E402


def fastq_text(n_bytes, read_len=15000, seed=1):
    """long reads: '@id', bases, '+', qualities with the skew of real ones (a few values carry most of the mass)"""
    rng = np.random.default_rng(seed)
    rec = read_len * 2 + 32
    n = max(1, n_bytes // rec)
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, read_len), p=[0.3, 0.2, 0.2, 0.3])
    qual = (33 + np.minimum(60, rng.geometric(0.4, (n, read_len)) + rng.integers(0, 3, (n, 1)) * 10)).astype(np.uint8)
    out = bytearray()
    for i in range(n):
        out += b"@m64011_%07d/%d/ccs\n" % (i, i * 7 % 1000); out += bases[i].tobytes(); out += b"\n+\n"; out += qual[i].tobytes(); out += b"\n"
    return bytes(out)


def fasta_text(n_bytes, seed=2):
    rng = np.random.default_rng(seed)
    lines = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_bytes // 61, 61))
    lines[:, 60] = 10
    body = lines.tobytes()
    out, at, i = bytearray(), 0, 0
    while at < len(body):
        out += b">contig_%d\n" % i; out += body[at:at + 61 * 20000]; at += 61 * 20000; i += 1
    return bytes(out)


def best(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter(); r = fn(); times.append(time.perf_counter() - t)
    return min(times), r


def kernel_rates(blob, text_len, reps):
    members = mg.bgzf_members(blob)
    tab = (mg.MgGzMember * len(members))(*[mg.MgGzMember(c, u, cl, ul, crc, 0) for c, cl, u, ul, crc in members])
    d_comp, d_out = mg.DeviceBuffer.from_numpy(np.frombuffer(blob, np.uint8)), mg.DeviceBuffer(text_len)
    import ctypes as C
    out = {}
    for name, knob in (("crc", None), ("nocrc", 1)):
        with mg.knobs(INFLATE_NOCRC=knob):
            def run():
                bad = C.c_uint32(0)
                mg.check(mg.lib().mgInflateMembersDevice(d_comp.ptr, len(blob), tab, len(members), d_out.ptr, text_len, None, C.byref(bad), None))
                assert bad.value == 0
            t, _ = best(run, reps)
        out[name] = dict(seconds=t, text_gb_s=text_len / t / 1e9, diag=mg.inflate_diag())
    got = d_out.to_numpy(np.uint8, min(text_len, 1 << 20)).tobytes()
    d_comp.free(); d_out.free()
    return out, got, members


def zlib_threads(blob, members, threads, reps):
    view = memoryview(blob)

    def one(rng):
        n = 0
        for c, cl, u, ul, crc in members[rng[0]:rng[1]]:
            text = zlib.decompress(view[c:c + cl], -15, ul)
            assert zlib.crc32(text) == crc
            n += len(text)
        return n
    step = max(1, len(members) // (threads * 8))
    ranges = [(i, min(len(members), i + step)) for i in range(0, len(members), step)]
    with ThreadPool(threads) as pool:
        t, n = best(lambda: sum(pool.map(one, ranges)), reps)
    return dict(seconds=t, text_gb_s=n / t / 1e9, threads=threads)


def file_calls(paths, reps, new):
    out = {}
    cases = [("bgzf", paths["bgzf"], None), ("plain", paths["plain"], None)]
    if new:
        cases.insert(1, ("bgzf_host_knob", paths["bgzf"], 1))
    for name, path, knob in cases:
        with mg.knobs(**({"BGZF_HOST": knob} if new else {})):
            t, r = best(lambda: mg.composition_file(path, mg.COMP_BASES | mg.COMP_QUALS | mg.COMP_LENGTHS), reps)
            out["composition_" + name] = dict(seconds=t, diag=mg.inflate_diag() if new else None, n_seq=int(r[2]["nSeq"]), tot_len=int(r[2]["totLen"]))
            dst = paths["plain"] + ".out.fa"
            t, r = best(lambda: mg.seq_convert_file(path, dst, mg.SEQ_FASTA), reps)
            out["seqconvert_" + name] = dict(seconds=t, diag=mg.inflate_diag() if new else None, n_seq=r[1]["nSeq"], out_bytes=os.path.getsize(dst))
            os.remove(dst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--keep", action="store_true", help="leave the files where they are (for a second run on them)")
    ap.add_argument("--calls-only", action="store_true", help="only the file calls, on files a run with --keep left (an older library: MODGPU_LIB)")
    a = ap.parse_args()
    new = hasattr(mg.lib(), "mgInflateMembersDevice")
    result = dict(gib=a.gib, library="this tree" if not os.environ.get("MODGPU_LIB") else os.environ["MODGPU_LIB"])
    for kind, make, share in (("fastq", fastq_text, 1.0), ("fasta", fasta_text, 0.5)):
        paths = dict(plain=os.path.join(a.dir, "inflate_probe." + kind), bgzf=os.path.join(a.dir, "inflate_probe.%s.gz" % kind))
        r = dict()
        if not a.calls_only:
            text = make(int(a.gib * share * (1 << 30)))
            t = time.perf_counter(); blob = mg.bgzf_bytes(text, level=6, threads=16); r["deflate_seconds"] = time.perf_counter() - t
            open(paths["plain"], "wb").write(text); open(paths["bgzf"], "wb").write(blob)
            r.update(text_bytes=len(text), bgzf_bytes=len(blob))
            r["kernel"], head, members = kernel_rates(blob, len(text), a.reps)
            assert head == text[:len(head)]
            r["members"] = len(members)
            r["zlib_16_threads"] = zlib_threads(blob, members, 16, a.reps)
            del text, blob
        r["calls"] = file_calls(paths, a.reps, new)
        if not a.keep:
            os.remove(paths["plain"]); os.remove(paths["bgzf"])
        result[kind] = r
        print(kind, json.dumps(r), flush=True)
    if a.json:
        json.dump(result, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
