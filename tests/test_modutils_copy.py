"""modutils -s / -sM and the summary on a set WITHOUT a device table (modutils.c:205-219, modset.c:130-153): mgModsetSetCopy,
mgModsetSetCopyM and mgModsetSummaryDevice take the host arrays then, and no HIP device is needed.  The sets are the reference
program's own (tests/golden/tenx_*.mod, made by make_golden_tenx.py with -s 2 3 6 -sM 5), read with modsetRead."""
import gzip

import numpy as np
import pytest

import modimizer_amd as mg
import tenx_util as tx
from tenx_util import COPY, COPY_M, chain, host_summary

TAGS = list(tx.TAGS)
INPUTS = ["fq", "fa"]


def load_golden(tag, ext, tmp_path):
    p = str(tmp_path / "g.mod")
    open(p, "wb").write(gzip.open(tx.gpath("tenx_%s_%s.mod" % (tag, ext))).read())
    with mg.CFile(p, "r") as f:
        ms = mg.lib().modsetRead(f)
    assert not mg.lib().mgModsetDeviceSlots(ms)
    return ms


@pytest.mark.parametrize("ext", INPUTS)
@pytest.mark.parametrize("tag", TAGS)
def test_set_copy_matches_reference(tag, ext, tmp_path):
    ms = load_golden(tag, ext, tmp_path)
    depth, info = tx.host_views(ms)
    golden_info = info.copy()
    _, (after_x, after_s, after_sm) = tx.golden_lines(tag, ext)
    assert host_summary(ms, str(tmp_path / "h.txt")) == after_sm
    info[:] = 0                                                    # the set as -x left it
    assert mg.summary_device(ms, str(tmp_path / "s0.txt")) == after_x
    assert mg.set_copy(ms, *COPY) == 1
    assert np.array_equal(info[1:], chain(depth[1:], *COPY))
    assert mg.summary_device(ms, str(tmp_path / "s1.txt")) == after_s
    assert mg.set_copy_m(ms, COPY_M) == 1
    assert np.array_equal(info, golden_info)
    assert mg.summary_device(ms, str(tmp_path / "s2.txt")) == after_sm == host_summary(ms, str(tmp_path / "h2.txt"))
    mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("thr", [(-5, -1, 0), (0, 0, 0), (70000, 80000, 90000), (3, 70000, 4), (6, 3, 2), (4, 2, 9), (1, 65535, 65536), (2, 2, -7)])
def test_thresholds_of_any_order_follow_the_chain(thr, tmp_path):
    ms = load_golden("k11w4", "fq", tmp_path)
    depth, info = tx.host_views(ms)
    depth[1] = 65535; depth[2] = 0                                 # both ends of the range are there
    rng = np.random.default_rng(5)
    high = (rng.integers(0, 64, len(info)) << 2).astype(np.uint8)  # bits 2 .. 7, kept by both commands
    info[:] = high | (info & 3)
    info[0] = 0xab; depth[0] = 77                                  # entry 0 is no entry: never written
    assert mg.set_copy(ms, *thr) == 1
    want = high[1:] | chain(depth[1:], *thr)
    assert np.array_equal(info[1:], want) and info[0] == 0xab and depth[0] == 77
    # -sM only sets bits: where the depth reaches the threshold
    for m in (thr[0], thr[2], 4, 65535, 65536, -1):
        before = info.copy()
        assert mg.set_copy_m(ms, m) == 1
        assert np.array_equal(info[1:], np.where(depth[1:].astype(np.int64) >= m, before[1:] | 3, before[1:])) and info[0] == 0xab
    assert np.array_equal(info[1:] >> 2, high[1:] >> 2)
    assert mg.summary_device(ms, str(tmp_path / "d.txt")) == host_summary(ms, str(tmp_path / "h.txt"))
    mg.lib().modsetDestroy(ms)


def test_summary_of_an_empty_set(tmp_path):
    ms = mg.modsetCreate(mg.seqhashCreate(19, 31, 17), 20)
    text = mg.summary_device(ms, str(tmp_path / "d.txt"))
    assert text == host_summary(ms, str(tmp_path / "h.txt"))
    assert text.splitlines()[-1] == "MS table bits 20 size 1048576 number of entries 0"
    assert mg.set_copy(ms, 1, 2, 3) == 1 and mg.set_copy_m(ms, 1) == 1
    assert ms.contents.info[0] == 0
    mg.lib().modsetDestroy(ms)
