"""dev probe: modasm -R / -T (mgReadsetRefFlagFile, mgReadsetTestMods) on a set of the golden maker's design (tests/golden/make_golden_rdna.py: a tandem
array, variant units, two haplotypes, reads on both strands) with a longer unit, so more mods per unit, more hits per read and more tested mods: on the
device with and without the ZZ-TEST lines, by the library's host loops, and by the reference program (oracle/_ref/modasm_ref -r stem -R ref -C -T lo hi,
less what -r -R -C alone take; it always writes both files).  Every timed call runs on a fresh load of the set.  Prints the runs, the counters of
mgReadsetRdnaDiag and one JSON line.
--no-clean leaves the -C out, so that the unit's own mods (depth 2751 .. 4750) can be tested: thousands of visits per tested mod.
usage: python tools/rdna_probe.py [--unit BASES] [--lo D] [--hi D] [--runs R] [--no-ref] [--no-clean] [out.json]"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import modimizer_amd as mg  # noqa: E402
from modimizer_amd import fasta  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
spec = importlib.util.spec_from_file_location("make_golden_rdna", os.path.join(ROOT, "tests", "golden", "make_golden_rdna.py"))
maker = importlib.util.module_from_spec(spec); spec.loader.exec_module(maker)


def wall(cmd, cwd):
    t = time.perf_counter()
    subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return time.perf_counter() - t


def lib_run(stem, ref, lo, hi, d, with_z, host, clean=True):
    """(seconds of -R, seconds of -T, path, diag) on a fresh load; -C between, as the reference run has it"""
    L = mg.lib()
    with mg.knobs(READSET_HOST=1 if host else None):
        rs = L.mgReadsetLoad(stem.encode())
        with mg.CFile(os.path.join(d, "o.txt"), "w") as f, mg.CFile(os.path.join(d, "y.txt"), "w") as y, mg.CFile(os.path.join(d, "z.txt"), "w") as z:
            t0 = time.perf_counter(); mg.readset_ref_flag(rs, ref, f); t1 = time.perf_counter()
            if clean:
                L.mgReadsetCleanMods(rs, f)
            t2 = time.perf_counter(); path = mg.readset_test_mods(rs, lo, hi, f, y, z if with_z else None); t3 = time.perf_counter()
        diag = mg.readset_rdna_diag()
        L.mgReadsetDestroy(rs)
    return t1 - t0, t3 - t2, path, diag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unit", type=int, default=240); ap.add_argument("--lo", type=int, default=2); ap.add_argument("--hi", type=int, default=400)
    ap.add_argument("--runs", type=int, default=3); ap.add_argument("--no-ref", action="store_true"); ap.add_argument("--no-clean", action="store_true"); ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    k, w = 19, 8
    d = tempfile.mkdtemp()
    sn, ss, rn, rr, refs = maker.make_inputs(a.unit)
    fasta.write_fasta(os.path.join(d, "src.fa"), sn, ss); fasta.write_fasta(os.path.join(d, "reads.fa"), rn, rr)
    fasta.write_fasta(os.path.join(d, "ref.fa"), *refs["_ref"][:2])
    MU, MA = os.path.join(REF, "modutils_ref"), os.path.join(REF, "modasm_ref")
    subprocess.run([MU, "-c", "22", str(k), str(w), "17", "-a", "src.fa", "-s", "1", "2", "3", "-w", "src.mod"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    subprocess.run([MA, "-m", "src.mod", "-f", "reads.fa", "-w", "set"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    stem, ref = os.path.join(d, "set"), os.path.join(d, "ref.fa")
    res = {"unit": a.unit, "reads": len(rr), "bases": int(sum(len(r) for r in rr)), "lo": a.lo, "hi": a.hi}
    clean = not a.no_clean
    lib_run(stem, ref, a.lo, a.hi, d, True, False, clean)                                  # warm-up: the device, the library's buffers
    for name, with_z, host in (("device_z", True, False), ("device", False, False), ("host_z", True, True), ("host", False, True)):
        runs = [lib_run(stem, ref, a.lo, a.hi, d, with_z, host, clean) for _ in range(a.runs)]
        res[name] = {"R_s": sorted(round(r[0], 4) for r in runs), "T_s": sorted(round(r[1], 4) for r in runs), "path": runs[0][2], "diag": runs[0][3]}
        print(name, res[name], flush=True)
    if not a.no_ref:
        base = ["-r", "set"]
        t_r = [wall([MA] + base, d) for _ in range(a.runs)]
        t_rr = [wall([MA] + base + ["-R", "ref.fa"], d) for _ in range(a.runs)]
        c = ["-C"] if clean else []
        t_rc = [wall([MA] + base + ["-R", "ref.fa"] + c, d) for _ in range(a.runs)]
        t_rt = [wall([MA] + base + ["-R", "ref.fa"] + c + ["-T", str(a.lo), str(a.hi)], d) for _ in range(a.runs)]
        med = lambda v: sorted(v)[len(v) // 2]
        res["reference"] = {"R_s": round(med(t_rr) - med(t_r), 4), "T_s": round(med(t_rt) - med(t_rc), 4), "whole_s": round(med(t_rt), 4)}
        print("reference", res["reference"], flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
