"""modutils -d / -P (mgReportDepths, mgRefPaint, mgRefPaintFile): the ABI and the behaviour without a device (CPU suite)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import modimizer_amd as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mgReportDepths", "mgRefPaint", "mgRefPaintFile"]


def test_report_functions_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert hasattr(L, n), n
        assert n in mg.EXPORTS, n
        assert getattr(L, n).restype is C.c_int
    for f in ("report_depths", "refpaint_file", "refpaint"):
        assert callable(getattr(mg, f))


def test_report_kernels_have_profile_names():
    L = mg.lib()
    names = set()
    for i in range(L.mgProfileKernels()):
        nm, ms, n = C.c_char_p(), C.c_double(), C.c_uint64()
        assert L.mgProfileGet(i, C.byref(nm), C.byref(ms), C.byref(n)) == 0
        names.add(nm.value.decode())
    for k in ("mgPaintItemsKernel", "mgDepthGuardKernel", "mgDepthGatherKernel", "mgTextLenKernel", "mgTextScanKernel", "mgTextWriteKernel"):
        assert k in names, k


def test_unreadable_paint_file_gives_the_reference_message(tmp_path):
    L = mg.lib()
    sh = mg.seqhashCreate(21, 64, 17)
    ms = mg.modsetCreate(sh, 20)
    missing = str(tmp_path / "no_such.fa")
    with pytest.raises(mg.ModgpuError, match="failed to open ref seq file %s" % re.escape(missing)):
        mg.refpaint_file(ms, missing, str(tmp_path / "out.txt"))
    assert L.mgLastError().decode() == "failed to open ref seq file %s" % missing
    assert ms.contents.max == 0
    L.modsetDestroy(ms)


no_gpu = pytest.mark.skipif(mg.lib().mgDeviceCount() > 0, reason="checks the no-device behaviour")


@no_gpu
def test_reports_fail_loudly_without_device(tmp_path):
    L = mg.lib()
    sh = mg.seqhashCreate(21, 64, 17)
    ms = mg.modsetCreate(sh, 20)
    other = mg.modsetCreate(mg.seqhashCreate(21, 64, 17), 20)
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.report_depths(ms, [other], str(tmp_path / "d.txt"))
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.report_depths(ms, [], str(tmp_path / "d0.txt"))
    fa = tmp_path / "r.fa"
    fa.write_text(">r1\nACGTACGTACGTACGTACGTACGTACGT\n")
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.refpaint_file(ms, str(fa), str(tmp_path / "p.txt"))
    bases = np.zeros(50, np.uint8)
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.refpaint(ms, bases, np.array([0, 50], np.int64), ["r1"], str(tmp_path / "p2.txt"))
    assert L.mgRefPaint(ms, None, None, 0, None, None) == -1
    L.modsetDestroy(ms); L.modsetDestroy(other)
