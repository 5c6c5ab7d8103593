"""modutils -s / -sM and the set summary on the GPU (modutils.c:205-219, modset.c:130-153): mgModsetSetCopy, mgModsetSetCopyM and
mgModsetSummaryDevice on a set whose depths are where the device table keeps them -- pending counts, synced ones, a table made from a
.mod -- against the reference program's files (tests/golden/tenx_*), and against the host arrays once they are synced.  Every call
asserts that it ran on the device (mgModsetSetCopyPath), that the array transfers' team moved info[] up and down and nothing else
(mgXferDiag), and that the table still holds what a later modsetSyncToHost has to bring."""
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
import util
import tenx_util as tx

pytestmark = pytest.mark.gpu
STATES = ["pending", "synced", "loaded"]


def build_state(tag, ext, state, tmp_path):
    """the set of `modutils -c B k w s -x reads` in one of three states: 'pending' (built on the device, nothing synced), 'synced'
    (modsetSyncToHost), 'loaded' (written, read back with modsetRead, and given a device table from its host arrays)"""
    L = mg.lib()
    ms = tx.new_set(tag)
    mg.add_sequence_file_10x(ms, tx.gpath("tenx_reads." + ext), str(tmp_path / "added.txt"))
    if state == "synced":
        mg.check(L.modsetSyncToHost(ms, 1))
    elif state == "loaded":
        p = str(tmp_path / "cur.mod")
        with mg.CFile(p, "w") as f:
            L.modsetWrite(ms, f)
        tx.destroy(ms)
        with mg.CFile(p, "r") as f:
            ms = L.modsetRead(f)
        assert not L.mgModsetDeviceSlots(ms)
        mg.write_text_device(ms, str(tmp_path / "make_table.txt"))      # (a set without a device table gets one)
    assert L.mgModsetDeviceSlots(ms)
    return ms


def on_device(call, *args):
    """call (*args) ran on the device, and the transfers' team moved two arrays: info[] up, info[] down"""
    before = util.xfer_diag()["transfers"]
    assert call(*args) == 0
    assert util.xfer_diag()["transfers"] - before == 2
    return True


@pytest.mark.parametrize("route", ["direct", "bucket"])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("ext", ["fq", "fa"])
def test_set_copy_in_three_states_matches_reference(ext, state, route, tmp_path):
    """route: how the table was built -- 'bucket': one bucketed add into an empty table, whose merge kernel kept the live histogram
    mgTableHistogram then starts from (pending state only: a sync or a load ends it); 'direct': by atomics, the histogram walks the table"""
    L = mg.lib()
    tag = "k11w4" if ext == "fq" else "k25w3"
    _, (after_x, after_s, after_sm) = tx.golden_lines(tag, ext)
    _, gmax, gvalue, gdepth, ginfo = tx.golden_mod(tag, ext)
    with mg.knobs(TABLE_PATH=route):
        ms = build_state(tag, ext, state, tmp_path)
    slots = L.mgModsetDeviceSlots(ms)
    assert mg.summary_device(ms, str(tmp_path / "s0.txt")) == after_x
    _, info = tx.host_views(ms)
    info[0] = 0x5a                                              # entry 0 is no entry: never written, on either side
    assert on_device(mg.set_copy, ms, *tx.COPY)
    _, info = tx.host_views(ms)
    assert ms.contents.max == gmax and np.array_equal(info[1:], tx.chain(gdepth[1:], *tx.COPY)) and info[0] == 0x5a
    assert mg.summary_device(ms, str(tmp_path / "s1.txt")) == after_s
    assert on_device(mg.set_copy_m, ms, tx.COPY_M)
    assert np.array_equal(tx.host_views(ms)[1][1:], ginfo[1:])
    assert mg.summary_device(ms, str(tmp_path / "s2.txt")) == after_sm
    assert L.mgModsetDeviceSlots(ms) == slots
    if state == "pending":                                      # nothing has reached the host's depth[] yet ...
        assert not tx.host_views(ms)[0].any()
    mg.check(L.modsetSyncToHost(ms, 1))                         # ... and the table still holds all of it
    v, d, f = mg.modset_arrays(ms)
    assert np.array_equal(v[1:], gvalue[1:]) and np.array_equal(d[1:], gdepth[1:]) and np.array_equal(f[1:], ginfo[1:])
    assert tx.host_summary(ms, str(tmp_path / "h.txt")) == after_sm
    tx.destroy(ms)


def check_copy(ms, thr, m, tmp_path):
    """-s thr and -sM m on the device against the chain on the depths a sync brings afterwards; info bits 2 .. 7 kept"""
    L = mg.lib()
    n = ms.contents.max + 1
    rng = np.random.default_rng(n)
    high = (rng.integers(0, 64, n) << 2).astype(np.uint8)
    info = np.ctypeslib.as_array(ms.contents.info, (n,))
    info[:] = high | (info & 3)
    assert on_device(mg.set_copy, ms, *thr)
    after_s = np.ctypeslib.as_array(ms.contents.info, (n,)).copy()
    dev_s = mg.summary_device(ms, str(tmp_path / "cs.txt"))
    assert on_device(mg.set_copy_m, ms, m)
    after_m = np.ctypeslib.as_array(ms.contents.info, (n,)).copy()
    dev_m = mg.summary_device(ms, str(tmp_path / "cm.txt"))
    mg.check(L.modsetSyncToHost(ms, 0))
    depth = np.ctypeslib.as_array(ms.contents.depth, (n,)).copy()
    assert np.array_equal(after_s[1:], high[1:] | tx.chain(depth[1:], *thr)) and after_s[0] == high[0]
    assert np.array_equal(after_m[1:], np.where(depth[1:].astype(np.int64) >= m, after_s[1:] | 3, after_s[1:])) and after_m[0] == high[0]
    assert dev_m == tx.host_summary(ms, str(tmp_path / "ch.txt"))
    info[:] = after_s
    assert dev_s == tx.host_summary(ms, str(tmp_path / "ch2.txt"))
    info[:] = after_m
    return depth


def test_depths_at_every_threshold_and_thresholds_of_any_order(tmp_path):
    """reads of their own k-mers repeated c1 - 1, c1, c2 - 1, c2, cM - 1 and cM times; then thresholds negative, above 65535 and out of order"""
    L = mg.lib()
    c1, c2, cm = 3, 6, 9
    rng = np.random.default_rng(77)
    reads = []
    for times in (c1 - 1, c1, c2 - 1, c2, cm - 1, cm):
        r = rng.integers(0, 4, 80).astype(np.uint8)
        reads += [r] * times
    ms = mg.modsetCreate(mg.seqhashCreate(15, 3, 17), 20)
    bases, offs = util.concat_reads(reads)
    mg.add_sequence_batch(ms, bases, offs)
    depth = check_copy(ms, (c1, c2, cm), cm, tmp_path)
    assert set(depth[1:].tolist()) >= {c1 - 1, c1, c2 - 1, c2, cm - 1, cm}
    mg.add_sequence_batch(ms, bases[:400], offs[:6])                    # pending counts on top of the synced ones
    for thr, m in (((-5, -1, 0), -3), ((70000, 80000, 90000), 65536), ((6, 3, 2), 2), ((3, 70000, 4), 65535), ((0, 0, 0), 0)):
        check_copy(ms, thr, m, tmp_path)
    tx.destroy(ms)


def test_saturated_depth(tmp_path):
    """70 000 copies of one read of 40 bases: the pending count of each of its modimizers is past 16 bits, its depth 65535"""
    L = mg.lib()
    read = "ACGTTGCATCGGATCCTAGACTGATCGTAACGTTAGCCAT"
    path = str(tmp_path / "many.fa")
    with open(path, "w") as f:
        f.write((">r\n" + read + "\n") * 70000)
    ms = mg.modsetCreate(mg.seqhashCreate(11, 2, 17), 20)
    with mg.CFile(str(tmp_path / "a.txt"), "w") as f:
        assert L.mgAddSequenceFile(ms, path.encode(), f) == 0
    depth = check_copy(ms, (65535, 65536, 70000), 65535, tmp_path)
    assert ms.contents.max >= 1 and np.all(depth[1:] == 65535)
    assert np.all(np.ctypeslib.as_array(ms.contents.info, (ms.contents.max + 1,))[1:] & 3 == 3)
    tx.destroy(ms)


def test_after_pruning_and_after_merging(tmp_path):
    L = mg.lib()
    tag = "k11w4"
    ms = build_state(tag, "fq", "pending", tmp_path)
    L.modsetDepthPrune(ms, 2, 9)
    assert 0 < ms.contents.max < tx.golden_mod(tag, "fq")[1]
    depth = check_copy(ms, tx.COPY, tx.COPY_M, tmp_path)
    assert depth[1:].min() >= 2 and depth[1:].max() < 9
    other = build_state(tag, "fa", "synced", tmp_path)
    mx = ms.contents.max
    assert L.modsetMerge(ms, other)
    assert ms.contents.max > mx and L.mgModsetDeviceSlots(ms)
    with mg.CFile(str(tmp_path / "b.txt"), "w") as f:                      # and pending counts on top of the merged depths
        assert L.mgAddSequenceFile(ms, tx.gpath("tenx_reads.fa").encode(), f) == 0
    check_copy(ms, (3, 5, 8), 6, tmp_path)
    tx.destroy(other)
    tx.destroy(ms)


def test_example_tenx_file(tmp_path):
    """examples/tenx_file.c: modutils -c B k w s -x reads.fq -s a b c -sM m -H his -wt out, against the reference's stdout and files"""
    tag, ext = "k11w4", "fq"
    exe = str(tmp_path / "tenx_file")
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "include"),
                        os.path.join(util.ROOT, "examples", "tenx_file.c"), "-o", exe, "-L", libdir, "-lmodgpu",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    B, k, w, s = tx.TAGS[tag]
    r = subprocess.run([exe, "-c", str(B), str(k), str(w), str(s), "-x", tx.gpath("tenx_reads." + ext), "-s"] + [str(c) for c in tx.COPY]
                       + ["-sM", str(tx.COPY_M), "-H", str(tmp_path / "his.txt"), "-wt", str(tmp_path / "out.txt")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    assert r.stdout == util.golden_text("tenx_%s_%s.stdout.txt" % (tag, ext))
    assert open(tmp_path / "his.txt").read() == util.golden_text("tenx_%s_%s.hist.txt" % (tag, ext))
    assert open(tmp_path / "out.txt").read() == util.golden_text("tenx_%s_%s.dump.txt" % (tag, ext))
