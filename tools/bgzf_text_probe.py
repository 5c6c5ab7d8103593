#!/usr/bin/env python3
"""dev probe (GPU): blocked-gzip (BGZF) FASTA / FASTQ through the device text parser at size.  Two synthetic files in tmpfs, about 1 GB of text
each -- FASTA of 10 kb reads, FASTQ of 150 b reads, as tools/composition_probe.py builds its own -- each as plain text and as BGZF
(mg.bgzf_bytes, 65280-byte blocks, level 6).  For each: wall time and Gbp/s of mgAddSequenceFile (k = 21, d = 64, seed 17) and of
mgReferenceFastaRead + mgQueryFile (the query alone is timed), three ways:
  bgzf_device   the BGZF file, inflated and parsed on the device;
  bgzf_host     the same file with MODGPU_BGZF_HOST=1: the host's inflate pool and parser, the path before the device took such files
                (--parent-lib: the same once more through another build of the library, to confirm that);
  plain         the plain file;
and for the query plain_ids_device: the plain file with MODGPU_TEXT_IDS_DEVICE=1, the id kernels against the host team on the same text.
Every (file, way) runs in a process of its own (the knobs are the process's environment) with MODGPU_TEXT_TIMING=1: one warm-up call, then
the repeats; median, least and greatest wall time; the phase lines of the last repeat.  Writes profiles/bgzf_text_probe.json.
usage: bgzf_text_probe.py [--gb 1] [--repeats 3] [--dir /dev/shm] [--parent-lib path/to/libmodgpu.so]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(call, path, ref, repeats):
    import modimizer_amd as mg
    L = mg.lib()
    times = []
    for r in range(repeats + 1):                             # the first is the warm-up: buffers, page cache
        sh = mg.seqhashCreate(21, 64, 17); ms = mg.modsetCreate(sh, 26)
        sys.stderr.write("== repeat %d\n" % r); sys.stderr.flush()
        with mg.CFile("/dev/null", "w") as f:
            if call == "add":
                t0 = time.perf_counter()
                rc = L.mgAddSequenceFile(ms, path.encode(), f)
                t = time.perf_counter() - t0
            else:
                rf = L.mgReferenceCreate(ms, 1 << 26)
                assert L.mgReferenceFastaRead(rf, ref.encode(), True, f) == 0
                t0 = time.perf_counter()
                rc = L.mgQueryFile(rf, path.encode(), f)
                t = time.perf_counter() - t0
                L.mgReferenceDestroy(rf)
        assert rc == 0, L.mgLastError()
        L.modsetDestroy(ms)
        if r:
            times.append(t)
    row = {"seconds": round(statistics.median(times), 4), "seconds_min_max": [round(min(times), 4), round(max(times), 4)]}
    if hasattr(L, "mgTextFileDiag"):
        row["diag"] = mg.text_file_diag(); row["inflate"] = mg.inflate_diag()
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.child[2], a.repeats)
    import modimizer_amd as mg
    from composition_probe import write_fasta, write_fastq
    rng = np.random.default_rng(7)
    stem = os.path.join(a.dir, "bgzf_text_probe_%d" % os.getpid())
    ref = stem + ".ref.fa"
    made = [ref]
    out = {"gb": a.gb, "repeats": a.repeats}
    try:
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), 4_000_000)
        open(ref, "wb").write(b">ref\n" + b"\n".join(s[i:i + 80].tobytes() for i in range(0, len(s), 80)) + b"\n")
        for kind, write, ext, per_rec, rec_bytes in (("fasta", write_fasta, "fa", 10000, None), ("fastq", write_fastq, "fq", 150, None)):
            plain, bgz = "%s.%s" % (stem, ext), "%s.%s.gz" % (stem, ext)
            made += [plain, bgz]
            size = write(plain, int(a.gb * 1e9), rng, False)
            text = open(plain, "rb").read()
            bases = text.count(b"\n>") + 1 if kind == "fasta" else text.count(b"\n") // 4
            bases *= per_rec
            t0 = time.perf_counter(); blob = mg.bgzf_bytes(text, level=6, threads=16); enc = time.perf_counter() - t0
            open(bgz, "wb").write(blob)
            row = {"text_bytes": size, "bgzf_bytes": len(blob), "bases": bases, "encode_seconds": round(enc, 1)}
            del text, blob
            ways = [("bgzf_device", bgz, {}, ""), ("bgzf_host", bgz, {"MODGPU_BGZF_HOST": "1"}, ""), ("plain", plain, {}, "")]
            if a.parent_lib:
                ways.append(("bgzf_parent_build", bgz, {}, a.parent_lib))
            for call in ("add", "query"):
                for way, path, env, lib in ways + ([("plain_ids_device", plain, {"MODGPU_TEXT_IDS_DEVICE": "1"}, "")] if call == "query" else []):
                    e = dict(os.environ, MODGPU_TEXT_TIMING="1", **env)
                    if lib:
                        e["MODGPU_LIB"] = lib
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--child", call, path, ref],
                                       capture_output=True, text=True, env=e, timeout=900)
                    if r.returncode:
                        row["%s_%s" % (call, way)] = {"failed": r.stderr[-400:]}
                        continue
                    res = json.loads(r.stdout.strip().splitlines()[-1])
                    res["Gbp_per_s"] = round(bases / res["seconds"] / 1e9, 2)
                    res["Gbp_per_s_min_max"] = [round(bases / res["seconds_min_max"][1] / 1e9, 2), round(bases / res["seconds_min_max"][0] / 1e9, 2)]
                    last = r.stderr.rsplit("== repeat", 1)[-1]
                    res["phases"] = [l.strip() for l in last.splitlines() if "[device text]" in l or "[parse]" in l]
                    row["%s_%s" % (call, way)] = res
                    print(kind, call, way, res["seconds"], res["Gbp_per_s"], res["Gbp_per_s_min_max"], flush=True)
            out[kind] = row
            for p in (plain, bgz):
                os.unlink(p); made.remove(p)
    finally:
        for p in made:
            if os.path.exists(p):
                os.unlink(p)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "bgzf_text_probe.json"), "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
