"""dev probe: modutils -wt / -rt (mgModsetWriteTextDevice, mgModsetReadText) on a set of about N entries: wall time, kernel ms per id,
the library's phase lines (MODGPU_TEXT_TIMING / MODGPU_SEED_TIMING), the host loop mgModsetWriteText, examples/text_file.c as a whole
process, and the reference program (oracle/_ref/modutils_ref -rt ..., -rt ... -wt ...) on the same box and the same file.
One size per run, so that a job gives every step its own time limit; the figures are merged into the JSON file:

    python tools/text_probe.py ENTRIES out.json [--no-ref | --ref-if-under SECONDS]

ENTRIES < 5e7: that many random 21-mers (a tenth of them added twice); otherwise config 2's set (10 Gbp of synthetic reads, k=21 d=64).
--ref-if-under: the reference program is run only if the 1e7 figures already in out.json predict less than SECONDS for it (linear in the
entries); the prediction is recorded either way."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import modimizer_amd as mg  # noqa: E402
from report_probe import device_set, kernel_ms, stderr_to  # noqa: E402

MU = os.path.join(ROOT, "oracle", "_ref", "modutils_ref")


def random_set(L, n, bits):
    rng = np.random.default_rng(n)
    keys = np.unique(rng.integers(0, 1 << 42, int(n * 1.01), dtype=np.uint64))
    keys = keys[rng.permutation(len(keys))][:n]
    ms = mg.modsetCreate(mg.seqhashCreate(21, 64, 17), bits)
    for part in (keys, keys[::10]):
        d = mg.DeviceBuffer.from_numpy(part)
        mg.check(L.modsetAddBatchDevice(ms, d.ptr, len(part), None, 1, None))
        mg.check(L.mgStreamSynchronize(None))
        d.free()
    return ms


def timed(cmd, cwd):
    t = time.time()
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1500)
    assert r.returncode == 0, (cmd, r.stderr[-1000:])
    return round(time.time() - t, 3)


def main():
    n = int(float(sys.argv[1])); out = sys.argv[2]
    opt = sys.argv[3] if len(sys.argv) > 3 else ""
    allres = json.load(open(out)) if os.path.exists(out) else {}
    L = mg.lib()
    mg.check(L.mgSetDevice(0))
    work = tempfile.mkdtemp()
    res = {"scratch": os.path.dirname(work), "cpus": len(os.sched_getaffinity(0))}
    try:
        t = time.time()
        if n < 50_000_000:
            bits = 24 if n <= 4_000_000 else 26
            ms = random_set(L, n, bits)
        else:
            ms = device_set(L, 10_000_000_000, 333_333_333, 1000, 777)
        mg.check(L.modsetSyncToHost(ms, 1))
        res["build_s"] = round(time.time() - t, 2); res["entries"] = ms.contents.max
        dump, log = os.path.join(work, "dump.txt"), os.path.join(work, "lib.log")
        for rep in range(2):
            L.mgProfileReset(); L.mgProfileEnable(1)
            with mg.knobs(SEED_TIMING=1), stderr_to(log):
                t = time.time(); mg.write_text_device(ms, dump); dt = time.time() - t
            L.mgProfileEnable(0)
            res["write_device_%d" % rep] = {"wall_s": round(dt, 3), "kernels_ms": kernel_ms(L), "writer": open(log).read().strip()}
        res["bytes"] = os.path.getsize(dump)
        host = os.path.join(work, "host.txt")
        t = time.time()
        with mg.CFile(host, "w") as f:
            L.mgModsetWriteText(ms, f)
        res["write_host_loop_s"] = round(time.time() - t, 3)
        res["host_loop_same_bytes"] = subprocess.run(["cmp", "-s", dump, host]).returncode == 0
        os.remove(host)
        L.modsetDestroy(ms)
        for rep in range(2):                             # page cache warm: the file was just written
            L.mgProfileReset(); L.mgProfileEnable(1)
            with mg.knobs(TEXT_TIMING=1), stderr_to(log):
                t = time.time(); ms2 = mg.read_text(dump); dt = time.time() - t
            L.mgProfileEnable(0)
            res["read_%d" % rep] = {"wall_s": round(dt, 3), "path": mg.read_text_path(), "kernels_ms": kernel_ms(L), "phases": open(log).read().strip().splitlines()}
            t = time.time(); mg.check(L.modsetSyncToHost(ms2, 1)); res["read_%d" % rep]["sync_value_index_s"] = round(time.time() - t, 3)
            assert ms2.contents.max == res["entries"]
            L.modsetDestroy(ms2)
        # the same commands as whole processes: examples/text_file.c on the library, and the reference program
        exe = os.path.join(work, "text_file"); libdir = os.path.join(ROOT, "modimizer_amd")
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "text_file.c"), "-o", exe,
                               "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        res["example_rt_wt_process_s"] = timed([exe, "-rt", dump, "-wt", os.path.join(work, "ex.txt")], work)
        res["example_same_bytes"] = subprocess.run(["cmp", "-s", dump, os.path.join(work, "ex.txt")]).returncode == 0
        os.remove(os.path.join(work, "ex.txt"))
        run_ref = opt != "--no-ref" and os.path.exists(MU)
        if opt == "--ref-if-under":
            base = allres.get("10000000", {})
            if "ref_rt_s" in base:
                scale = res["entries"] / base["entries"]
                res["ref_predicted_from_1e7"] = {"rt_s": round(base["ref_rt_s"] * scale, 1), "rt_wt_s": round(base["ref_rt_wt_s"] * scale, 1)}
                run_ref = run_ref and base["ref_rt_wt_s"] * scale < float(sys.argv[4])
            else:
                run_ref = False
        if run_ref:
            res["ref_rt_s"] = timed([MU, "-o", "log.txt", "-rt", dump], work)
            res["ref_rt_wt_s"] = timed([MU, "-o", "log.txt", "-rt", dump, "-wt", "ref.txt"], work)
            res["ref_same_bytes"] = subprocess.run(["cmp", "-s", dump, os.path.join(work, "ref.txt")]).returncode == 0
            rd, wr = res["read_1"]["wall_s"], res["write_device_1"]["wall_s"]
            res["ratio_ref_over_new"] = {"rt": round(res["ref_rt_s"] / rd, 1), "rt_wt": round(res["ref_rt_wt_s"] / (rd + wr), 1),
                                         "wt_alone": round((res["ref_rt_wt_s"] - res["ref_rt_s"]) / wr, 1),
                                         "rt_wt_whole_process": round(res["ref_rt_wt_s"] / res["example_rt_wt_process_s"], 1)}
    finally:
        shutil.rmtree(work)
    allres.setdefault("box", "%s; %d CPUs visible; files under %s, page cache warm; one size per run, every launch bracketed by profile events"
                      % (L.mgVersion().decode(), res["cpus"], res["scratch"]))
    allres[str(n)] = res
    json.dump(allres, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
