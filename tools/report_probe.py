"""dev probe: modutils -d / -P (mgReportDepths, mgRefPaintFile) at config 2's size, where the time goes, against the unmodified
modutils.c on the library (oracle/_ref/modutils_dropin) and the reference program (oracle/_ref/modutils_ref) at a size they finish.
usage: python tools/report_probe.py [out_dir]   (GPU box; prints one table and the JSON of every figure)"""
import contextlib
import ctypes as C
import gzip
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

REF = os.path.join(ROOT, "oracle", "_ref")


@contextlib.contextmanager
def stderr_to(path):
    """the library's MODGPU_SEED_TIMING lines go to fd 2: catch them in a file"""
    sys.stderr.flush()
    save = os.dup(2)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2); os.close(fd)
    try:
        yield
    finally:
        os.dup2(save, 2); os.close(save)


def kernel_ms(L):
    out = {}
    for i in range(L.mgProfileKernels()):
        nm, ms, n = C.c_char_p(), C.c_double(), C.c_uint64()
        L.mgProfileGet(i, C.byref(nm), C.byref(ms), C.byref(n))
        if n.value:
            out[nm.value.decode()] = (round(ms.value, 3), n.value)
    return out


def device_set(L, total, G, plan_seed, err_seed, bits=30):
    starts, offs, strands = synth.ont_read_plan(total, G, plan_seed, n50=20000, sigma=0.6, lo=500, hi=200000)
    tot = int(offs[-1])
    d_g = mg.DeviceBuffer(L.mgPackedWords(G) * 4)
    mg.check(L.mgSynthGenome(d_g.ptr, G, 12345, None))
    d_s = mg.DeviceBuffer.from_numpy(starts); d_of = mg.DeviceBuffer.from_numpy(offs); d_st = mg.DeviceBuffer.from_numpy(strands)
    d_r = mg.DeviceBuffer(L.mgPackedWords(tot) * 4)
    mg.check(L.mgSynthReads(d_g.ptr, G, d_s.ptr, d_of.ptr, d_st.ptr, len(starts), tot, 0.05, err_seed, d_r.ptr, None))
    ms = mg.modsetCreate(mg.seqhashCreate(21, 64, 17), bits)
    n = C.c_uint64()
    mg.check(L.mgAddReadsDevice(ms, d_r.ptr, tot, d_of.ptr, len(starts), C.byref(n), None))
    mg.check(L.mgStreamSynchronize(None))
    for b in (d_g, d_s, d_of, d_st, d_r):
        b.free()
    return ms


def write_genome_fasta(L, path, nb, rec, seed=12345):
    d_g = mg.DeviceBuffer(L.mgPackedWords(nb) * 4)
    mg.check(L.mgSynthGenome(d_g.ptr, nb, seed, None))
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(path, "wb") as f:
        for r0 in range(0, nb, rec):
            n = min(rec, nb - r0)
            d_b = mg.DeviceBuffer(n + 16)
            src = C.c_void_p(d_g.ptr.value + r0 // 4)
            mg.check(L.mgUnpackDevice(src, n, d_b.ptr, None))
            f.write(b">c%d\n" % (r0 // rec)); f.write(lut[d_b.to_numpy(np.uint8, n)].tobytes() + b"\n")
            d_b.free()
    d_g.free()


def timed(cmd, cwd, out=None):
    t = time.time()
    r = subprocess.run(cmd, cwd=cwd, stdout=open(out, "w") if out else subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1800)
    assert r.returncode == 0, (cmd, r.stderr[-1000:])
    return time.time() - t


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    L = mg.lib()
    mg.check(L.mgSetDevice(0))
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 16e9 else None
    work = tempfile.mkdtemp(dir=shm)
    res = {"tmpfs": bool(shm)}
    try:
        # ---- -d at config 2's size ----
        t = time.time()
        ms = device_set(L, 10_000_000_000, 333_333_333, 1000, 777)
        ms2 = device_set(L, 10_000_000_000, 333_333_333, 2000, 778)
        res["build_s"] = round(time.time() - t, 1)
        res["entries"] = [ms.contents.max, ms2.contents.max]
        for rep in range(2):                             # the first call makes ms2's lookup layout; the second is the steady state
            L.mgProfileReset(); L.mgProfileEnable(1)
            p = os.path.join(work, "depths.txt"); log = os.path.join(work, "d.log")
            with mg.knobs(SEED_TIMING=1), stderr_to(log):
                t = time.time()
                mg.report_depths(ms, [ms2], p)
                dt = time.time() - t
            L.mgProfileEnable(0)
            res["depths_%d" % rep] = {"wall_s": round(dt, 3), "bytes": os.path.getsize(p), "kernels_ms": kernel_ms(L),
                                      "writer": open(log).read().strip()}
            os.remove(p)
        # ---- -P on 3 Gbp ----
        fa = os.path.join(work, "ref3g.fa")
        t = time.time(); write_genome_fasta(L, fa, 3_000_000_000, 50_000_000); res["fasta_write_s"] = round(time.time() - t, 1)
        for rep in range(2):
            L.mgProfileReset(); L.mgProfileEnable(1)
            p = os.path.join(work, "paint.txt"); log = os.path.join(work, "p.log")
            with mg.knobs(SEED_TIMING=1), stderr_to(log):
                t = time.time()
                mg.refpaint_file(ms, fa, p)
                dt = time.time() - t
            L.mgProfileEnable(0)
            res["paint_%d" % rep] = {"wall_s": round(dt, 3), "bytes": os.path.getsize(p), "kernels_ms": kernel_ms(L),
                                     "writer": [l for l in open(log).read().splitlines() if l.startswith("mgTextOut")]}
            os.remove(p)
        os.remove(fa)
        L.modsetDestroy(ms); L.modsetDestroy(ms2)

        # ---- the same work at a size the host programs finish: 200 Mbp of reads, 20 Mbp of reference ----
        G = 6_666_667
        genome = synth.iid_bases(G, 4242)
        for name, tot, ps, es in (("reads.fa", 200_000_000, 11, 12), ("reads2.fa", 200_000_000, 21, 22)):
            starts, offs, strands = synth.ont_read_plan(tot, G, ps, n50=20000, sigma=0.6, lo=500, hi=200000)
            b = synth.reads_from_genome(genome, starts, offs, strands, 0.05, es)
            lut = np.frombuffer(b"ACGT", np.uint8)
            with open(os.path.join(work, name), "wb") as f:
                for r in range(len(starts)):
                    f.write(b">r%d\n" % r); f.write(lut[b[offs[r]:offs[r + 1]]].tobytes() + b"\n")
        write_genome_fasta(L, os.path.join(work, "ref.fa"), 20_000_000, 5_000_000, seed=4242)
        base = ["-c", "24", "21", "64", "17", "-a", "reads.fa"]
        small = {}
        have = [x for x in ("modutils_ref", "modutils_dropin") if os.path.exists(os.path.join(REF, x))]
        if have:
            timed([os.path.join(REF, have[0]), "-o", "log.txt", "-c", "24", "21", "64", "17", "-a", "reads2.fa", "-w", "b.mod"], work)
            open(os.path.join(work, "b.plain"), "wb").write(gzip.open(os.path.join(work, "b.mod")).read())
        for x in have:
            exe = os.path.join(REF, x)
            a = timed([exe, "-o", "log.txt"] + base, work)
            pa = timed([exe, "-o", "log.txt"] + base + ["-P", "ref.fa"], work, os.path.join(work, "p_%s.txt" % x))
            da = timed([exe, "-o", "log.txt"] + base + ["-d", "d_%s.txt" % x, "b.plain"], work)
            small[x] = {"add_s": round(a, 3), "paint_s": round(pa - a, 3), "depths_s": round(da - a, 3)}
        # the library on the same files (the set built from the file, the other read from the reference's .mod)
        ms = mg.modsetCreate(mg.seqhashCreate(21, 64, 17), 24)
        with mg.CFile(os.path.join(work, "added.txt"), "w") as f:
            mg.check(L.mgAddSequenceFile(ms, os.path.join(work, "reads.fa").encode(), f))
        t = time.time(); mg.refpaint_file(ms, os.path.join(work, "ref.fa"), os.path.join(work, "p_lib.txt")); pl = time.time() - t
        lib_small = {"paint_s": round(pl, 3)}
        if have:
            with mg.CFile(os.path.join(work, "b.plain"), "r") as f:
                ob = L.modsetRead(f)
            mg.report_depths(ms, [ob], os.path.join(work, "d_lib.txt"))       # (makes ob's table)
            t = time.time(); mg.report_depths(ms, [ob], os.path.join(work, "d_lib.txt")); lib_small["depths_s"] = round(time.time() - t, 3)
            for x in have:                                  # (the programs' stdout ends in their "total resources used" line)
                ref_paint = "".join(l for l in open(os.path.join(work, "p_%s.txt" % x)) if not l.startswith("total resources"))
                lib_small["paint_same_as_" + x] = open(os.path.join(work, "p_lib.txt")).read() == ref_paint
                lib_small["depths_same_as_" + x] = open(os.path.join(work, "d_lib.txt")).read() == open(os.path.join(work, "d_%s.txt" % x)).read()
            L.modsetDestroy(ob)
        lib_small["entries"] = ms.contents.max
        lib_small["depths_bytes"] = os.path.getsize(os.path.join(work, "d_lib.txt")) if have else None
        lib_small["paint_bytes"] = os.path.getsize(os.path.join(work, "p_lib.txt"))
        L.modsetDestroy(ms)
        small["library"] = lib_small
        res["small_200Mbp_reads_20Mbp_ref"] = small
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res, indent=1))
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "report_probe.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
