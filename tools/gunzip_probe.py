#!/usr/bin/env python3
"""dev: what ordinary gzip on the device costs and gains (csrc/mg_gunzip.hip, mg_gzipsrc.hip).

Writes FASTQ (and FASTA) text, the same text as zlib level 6 gzip and as BGZF, and times, as medians with the spread of --runs runs, the runs
of the variants interleaved:
  - mgGzipInflateFile at every chunk size of --chunks (KiB) and every batch size of --batches, with mgGunzipDiag of each;
  - mgCompositionFile and mgSeqConvertFile on the gzip file on the device, under MODGPU_GZIP_HOST=1 (the path before), on the plain file and on
    the BGZF file (the ceiling); the results of the first two must agree;
  - the same two calls on gzip files of --sizes MB of text, device against host: the crossover MODGPU_GZIP_MIN_KB is set from;
  - the text parser's calls, mgAddSequenceFile and mgQueryFile, on the gzip file on the device (one walk: mgGzipSrcDiag's peak of resident compressed
    bytes with it), under MODGPU_GZIP_HOST=1 (the host parser, the path before), on the plain file and on the BGZF file; the "added" lines and the
    query outputs of the four must agree; and mgAddSequenceFile over --sizes, device against host.
--only parser: the last item alone (--only inflate: all but it).
usage: python tools/gunzip_probe.py [--mb 1000] [--fasta-mb 500] [--runs 5] [--only parser] [--out profiles/gunzip_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import modimizer_amd as mg  # noqa: E402


def fastq(n_bytes, seed=1, read_len=150):
    rng = np.random.default_rng(seed)
    n = max(1, n_bytes // (2 * read_len + 40))
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, read_len))]
    quals = np.clip(rng.normal(30, 8, (n, read_len)), 0, 40).astype(np.uint8) + 33
    recs = []
    for i in range(n):
        recs.append(b"@read%d/1 len=%d\n" % (i, read_len) + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n")
    return b"".join(recs)


def fasta(n_bytes, seed=2, contig=60000):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(max(1, n_bytes // contig)):
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, contig)].reshape(-1, 60)
        out.append(b">contig%d\n" % i + b"\n".join(r.tobytes() for r in seq) + b"\n")
    return b"".join(out)


def gz(text):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def timed(fn):
    t = time.perf_counter(); r = fn(); return time.perf_counter() - t, r


def med(xs):
    return dict(median_s=round(statistics.median(xs), 4), min_s=round(min(xs), 4), max_s=round(max(xs), 4), runs=len(xs))


def add_file(path, out):
    """mgAddSequenceFile into a fresh set (k = 21, one k-mer in 64, 2^26 slots): the call's seconds and the line it prints"""
    L = mg.lib()
    sh = mg.seqhashCreate(21, 64, 17); ms = mg.modsetCreate(sh, 26)
    with mg.CFile(out, "w") as f:
        t, rc = timed(lambda: L.mgAddSequenceFile(ms, path.encode(), f))
    L.modsetDestroy(ms)
    assert rc == 0, L.mgLastError()
    return t, open(out).read()


def query_file(ref, path, out):
    L = mg.lib()
    with mg.CFile(out, "w") as f:
        assert L.mgQueryFile(ref, path.encode(), f) == 0, L.mgLastError()
    return os.path.getsize(out), zlib.crc32(open(out, "rb").read())


def parser_legs(a, texts, paths, tmp, res):
    L = mg.lib()
    out = os.path.join(tmp, "pout")
    variants = [("gzip_device", "gzip", dict(GZIP_MIN_KB=0)), ("gzip_host", "gzip", dict(GZIP_HOST=1)), ("plain", "plain", {}), ("bgzf", "bgzf", {})]
    ref_fa = os.path.join(tmp, "ref.fa")
    open(ref_fa, "wb").write(texts["fa"][:8 << 20])
    sh = mg.seqhashCreate(21, 64, 17); ms = mg.modsetCreate(sh, 24)
    ref = L.mgReferenceCreate(ms, 1 << 26)
    with mg.CFile(out, "w") as f:
        assert L.mgReferenceFastaRead(ref, ref_fa.encode(), True, f) == 0
    for k in texts:
        ta = {v[0]: [] for v in variants}; tq = {v[0]: [] for v in variants}; lines = {}; outs = {}; walk = {}
        for _ in range(a.runs):
            for name, f, kn in variants:
                with mg.knobs(**kn):
                    t, lines[name] = add_file(paths[k][f], out); ta[name].append(t)
                    way = mg.text_file_diag()["path"]
                    if name == "gzip_device":
                        walk = dict(mg.gzip_src_diag(), file=os.path.getsize(paths[k][f]), path=way)
                    assert way == dict(gzip_device=3, gzip_host=0, plain=1, bgzf=2)[name], (name, way)
                    t, outs[name] = timed(lambda: query_file(ref, paths[k][f], out)); tq[name].append(t)
        assert len(set(lines.values())) == 1 and len(set(outs.values())) == 1, (lines, outs)
        res["parser"][k] = dict(add={n: med(v) for n, v in ta.items()}, query={n: med(v) for n, v in tq.items()}, one_walk=walk, added=lines["plain"].strip())
    L.mgReferenceDestroy(ref); L.modsetDestroy(ms)
    for mb in map(int, a.sizes.split(",")):
        p = os.path.join(tmp, "p%d.gz" % mb)
        cut = texts["fq"].rfind(b"\n@read", 0, mb << 20) + 1      # whole records: a text cut inside one is handed to the host parser, which inflates it again
        open(p, "wb").write(gz(texts["fq"][:cut]))
        td, th = [], []
        for _ in range(a.runs):
            with mg.knobs(GZIP_MIN_KB=0):
                td.append(add_file(p, out)[0])
            with mg.knobs(GZIP_HOST=1):
                th.append(add_file(p, out)[0])
        res["parser"]["crossover_add_%d_MB_text" % mb] = dict(gz_kb=os.path.getsize(p) >> 10, device=med(td), host=med(th))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1000); ap.add_argument("--fasta-mb", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5); ap.add_argument("--chunks", default="64,128,256,512"); ap.add_argument("--batches", default="512,2048,8192")
    ap.add_argument("--sizes", default="1,4,16,64"); ap.add_argument("--out", default=""); ap.add_argument("--only", default="", choices=["", "parser", "inflate"])
    a = ap.parse_args()
    flags = mg.COMP_BASES | mg.COMP_QUALS | mg.COMP_LENGTHS
    res = dict(device=mg.lib().mgDeviceCount(), files={}, inflate={}, calls={}, crossover={}, parser={})
    with tempfile.TemporaryDirectory() as tmp:
        texts = dict(fq=fastq(a.mb << 20), fa=fasta(a.fasta_mb << 20))
        paths = {}
        for k, t in texts.items():
            paths[k] = {"plain": os.path.join(tmp, k + ".txt"), "gzip": os.path.join(tmp, k + ".gz"), "bgzf": os.path.join(tmp, k + ".bgz")}
            open(paths[k]["plain"], "wb").write(t)
            open(paths[k]["gzip"], "wb").write(gz(t))
            mg.bgzf_deflate_file(paths[k]["plain"], paths[k]["bgzf"])
            res["files"][k] = {n: os.path.getsize(p) for n, p in paths[k].items()}
        out = os.path.join(tmp, "out")
        if a.only != "inflate":
            parser_legs(a, texts, paths, tmp, res)
        # mgGzipInflateFile over the chunk and batch sizes, interleaved
        grid = [(c, b) for c in map(int, a.chunks.split(",")) for b in map(int, a.batches.split(","))]
        for k in texts if a.only != "parser" else ():
            times = {g: [] for g in grid}; diag = {}
            for _ in range(a.runs):
                for c, b in grid:
                    with mg.knobs(GZIP_CHUNK_KB=c, GZIP_BATCH=b):
                        t, _ = timed(lambda: mg.gzip_inflate_file(paths[k]["gzip"], out))
                    times[c, b].append(t); diag[c, b] = mg.gunzip_diag()
            assert open(out, "rb").read() == texts[k]
            res["inflate"][k] = {"%d_%d" % g: dict(med(times[g]), gb_s=round(len(texts[k]) / statistics.median(times[g]) / 1e9, 3), diag=diag[g]) for g in grid}
        # the two calls: device, host, plain, BGZF
        variants = [("gzip_device", "gzip", dict(GZIP_MIN_KB=0)), ("gzip_host", "gzip", dict(GZIP_HOST=1)), ("plain", "plain", {}), ("bgzf", "bgzf", {})]
        for k in texts if a.only != "parser" else ():
            kind = mg.SEQ_FASTQ if k == "fq" else mg.SEQ_FASTA
            tc = {v[0]: [] for v in variants}; ts = {v[0]: [] for v in variants}; got = {}
            for _ in range(a.runs):
                for name, f, kn in variants:
                    with mg.knobs(**kn):
                        t, r = timed(lambda: mg.composition_file(paths[k][f], flags)); tc[name].append(t); got[name] = r[0]
                        t, r = timed(lambda: mg.seq_convert_file(paths[k][f], out, kind)); ts[name].append(t)
            assert got["gzip_device"] == got["gzip_host"] == got["plain"]
            res["calls"][k] = dict(composition={n: med(v) for n, v in tc.items()}, seqconvert={n: med(v) for n, v in ts.items()})
        # the crossover against the host path
        for mb in map(int, a.sizes.split(",")) if a.only != "parser" else ():
            p = os.path.join(tmp, "s%d.gz" % mb)
            open(p, "wb").write(gz(texts["fq"][:mb << 20]))
            td, th = [], []
            for _ in range(a.runs):
                with mg.knobs(GZIP_MIN_KB=0):
                    td.append(timed(lambda: mg.composition_file(p, flags))[0])
                with mg.knobs(GZIP_HOST=1):
                    th.append(timed(lambda: mg.composition_file(p, flags))[0])
            res["crossover"]["%d_MB_text" % mb] = dict(gz_kb=os.path.getsize(p) >> 10, device=med(td), host=med(th))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
