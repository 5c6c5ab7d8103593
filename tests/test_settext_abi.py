"""modutils -wt / -rt (mgModsetWriteTextDevice, mgModsetReadText, mgModsetReadTextPath): the ABI, the errors that need no device with
the reference's own texts (tests/golden/text_errors.json, made by make_golden_text.py), and the behaviour without a device (CPU suite)."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import modimizer_amd as mg
import util

ROOT = util.ROOT
CASES = {c["name"]: c for c in json.load(open(os.path.join(util.GOLDEN, "text_errors.json")))}
NO_DEVICE_NEEDED = ["missing_file", "mangled_header", "bits_19", "size_too_big", "size_negative", "k_32", "w_0"]


def test_text_functions_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    assert re.search(r"\bint\s+mgModsetWriteTextDevice\s*\(\s*Modset\s*\*\s*ms\s*,\s*FILE\s*\*\s*f\s*\)\s*;", hdr)
    assert re.search(r"\bModset\s*\*\s*mgModsetReadText\s*\(\s*const\s+char\s*\*\s*filename\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+mgModsetReadTextPath\s*\(\s*void\s*\)\s*;", hdr)
    for n in ("mgModsetWriteTextDevice", "mgModsetReadText", "mgModsetReadTextPath"):
        assert hasattr(L, n), n
        assert n in mg.EXPORTS, n
    assert L.mgModsetWriteTextDevice.restype is C.c_int and L.mgModsetReadTextPath.restype is C.c_int
    assert L.mgModsetReadText.restype is C.POINTER(mg.Modset)
    for f in ("write_text_device", "read_text", "read_text_path"):
        assert callable(getattr(mg, f))
    # the dynamic symbol table has them (they are not hidden like the glue behind them)
    out = subprocess.run(["nm", "-D", "--defined-only", mg.LIB_PATH], capture_output=True, text=True).stdout
    for n in ("mgModsetWriteTextDevice", "mgModsetReadText", "mgModsetReadTextPath"):
        assert re.search(r" T %s$" % n, out, flags=re.M), n
    for n in ("mgSetTextParseDevice", "mgSetTextFillDevice", "mgTextReadParallel", "mgTextWindowBytes"):
        assert not re.search(r" %s$" % n, out, flags=re.M), n


def test_text_kernels_have_profile_names():
    L = mg.lib()
    names = set()
    for i in range(L.mgProfileKernels()):
        nm, ms, n = C.c_char_p(), C.c_double(), C.c_uint64()
        assert L.mgProfileGet(i, C.byref(nm), C.byref(ms), C.byref(n)) == 0
        names.add(nm.value.decode())
    for k in ("mgSetTextLinesKernel", "mgSetTextScanKernel", "mgSetTextParseKernel", "mgSetTextLastKernel"):
        assert k in names, k


@pytest.mark.parametrize("name", NO_DEVICE_NEEDED)
def test_errors_that_need_no_device_carry_the_reference_text(name, tmp_path):
    """the file, its header and what seqhashCreate / modsetCreate would die() on are judged before a device is asked for"""
    L = mg.lib()
    case = CASES[name]
    assert case["from_reference"]
    path = str(tmp_path / ("%s.txt" % name))
    if case["input"] is not None:
        open(path, "w").write(case["input"])
    assert not L.mgModsetReadText(path.encode())
    assert L.mgLastError().decode() == case["message"].replace("<FILE>", path)
    assert L.mgModsetReadTextPath() == -1
    with pytest.raises(mg.ModgpuError, match=re.escape(case["message"].replace("<FILE>", path).strip())):
        mg.read_text(path)


def test_invalid_arguments():
    L = mg.lib()
    assert L.mgModsetWriteTextDevice(None, None) == -1
    assert not L.mgModsetReadText(None)


def test_example_compiles(tmp_path):
    exe = str(tmp_path / "text_file")
    libdir = os.path.join(ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "text_file.c"), "-o", exe, "-L", libdir, "-lmodgpu",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


no_gpu = pytest.mark.skipif(mg.lib().mgDeviceCount() > 0, reason="checks the no-device behaviour")


@no_gpu
def test_text_calls_fail_loudly_without_device(tmp_path):
    L = mg.lib()
    sh = mg.seqhashCreate(21, 64, 17)
    ms = mg.modsetCreate(sh, 20)
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.write_text_device(ms, str(tmp_path / "d.txt"))
    with mg.CFile(str(tmp_path / "d2.txt"), "w") as f:
        assert L.mgModsetWriteTextDevice(ms, f) == -1
    assert os.path.getsize(tmp_path / "d2.txt") == 0             # not even the header line
    # the host loop stays what it was: it needs no device
    with mg.CFile(str(tmp_path / "h.txt"), "w") as f:
        L.mgModsetWriteText(ms, f)
    assert open(tmp_path / "h.txt").read() == "modset bits 20 size 1 k 21 w 64 seed 17\n"
    L.modsetDestroy(ms)
    for good in ("text_dups.txt", "text_loose.txt", "text_long.txt"):
        assert not L.mgModsetReadText(os.path.join(util.GOLDEN, good).encode())
        assert b"no HIP device" in L.mgLastError()
        with pytest.raises(mg.ModgpuError, match="no HIP device"):
            mg.read_text(os.path.join(util.GOLDEN, good))
    empty = tmp_path / "empty.txt"
    empty.write_text("modset bits 20 size 1 k 21 w 64 seed 17\n")
    assert not L.mgModsetReadText(str(empty).encode()) and b"no HIP device" in L.mgLastError()
