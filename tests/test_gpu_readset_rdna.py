"""modasm -R / -T / -rb on the device (mg_rdna.hip): the recorded sequences of the reference program through the device path; read sets made by
design where the kernels can go wrong, and a few hundred randomized small ones, against the restatement of tests/test_readset_rdna.py (itself held
against the reference program there); the example against its golden.  Every test asserts that the device path ran (mgReadsetRdnaPath () == 0) and,
where it is about a boundary, that the set sits on it -- from the restatement's numbers, never assumed."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests import test_readset as trs
from tests import test_readset_rdna as trd

pytestmark = pytest.mark.gpu
RD, C1 = trd.MS_RDNA, 1
OK = RD | C1                                                          # passes checkMod
K, W = 19, 8


def device_run(rs, cmds, tmp, hits):
    """through the library's device path whatever the size of the call (unset, a -T that walks fewer than 2^21 hits takes the host loops) and the restatement"""
    with mg.knobs(READSET_HOST=0):
        r = trd.run_both(rs, cmds, str(tmp), hits)
        assert mg.lib().mgReadsetRdnaPath() == 0
    return r


@pytest.mark.parametrize("tag", list(trd.TAGS))
def test_reference_sequences_on_the_device(tag, golden_dir, tmp_path):
    """every recorded sequence, -R from the reference file (scan and lookups on the device), -T and -rb on the device: the reference's bytes"""
    with mg.knobs(READSET_HOST=0):
        trd.check_sequences_through_library(tag, golden_dir, tmp_path, 0, hits=False)


def test_small_calls_take_the_host_loops(tmp_path):
    """the path choice: a -T that walks fewer than 2^21 hits is the host loops' unless MODGPU_READSET_HOST=0; the same bytes either way"""
    rs = mixed_set(str(tmp_path / "m"))
    hits = (np.array([2, 3], np.uint32), np.array([10, 400], np.int32))
    trd.run_both(rs, ["-R", "x", "-T", "1", "1000"], str(tmp_path), hits)
    assert mg.lib().mgReadsetRdnaPath() == 1
    trd.destroy(rs)


# ---- -R: the n200 / m200 kernel ----

def n200_set(stem):
    """mods 1 .. 20 plain, 21 and 22 in the reference and, by the hits of these reads, core.  Reads by their number of qualifying hits q, fillers between"""
    rng = np.random.default_rng(5)
    reads, names = [], []

    def add(name, mods):
        reads.append((10 * len(mods) + 100, [(int(m), bool(rng.integers(0, 2)), 10) for m in mods])); names.append(name)

    def mixed(q, first_qualifies):
        mods = [21 + int(rng.integers(0, 2)) for _ in range(q)] + [int(rng.integers(1, 21)) for _ in range(q // 3 + 2)]
        mods = list(rng.permutation(mods))
        if first_qualifies != (mods[0] > 20):
            j = next(j for j, m in enumerate(mods) if (m > 20) == first_qualifies)
            mods[0], mods[j] = mods[j], mods[0]
        return mods
    for q in (199, 200, 399, 400, 401):
        add("q%d" % q, mixed(q, False)); add("q%d_at0" % q, mixed(q, True))
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 300):
        add("all%d" % n, [21 if n in (1023, 1025) else 22] * n)
    add("empty", [])
    info = [0] + [C1] * 22
    return trd.build_set(stem, K, W, 22, reads, info), names


def test_n200_kernel_at_its_counts(tmp_path):
    """exactly 199, 200, 399, 400 and 401 qualifying hits, with and without one at hit 0 (which the loop from the back never sees); reads of 1, 63, 64, 65,
    1023 .. 1025 hits; then -T over the mods the walks have flagged"""
    rs, names = n200_set(str(tmp_path / "n"))
    hits = (np.array([21, 22], np.uint32), np.array([100, 200], np.int32))
    r = device_run(rs, ["-R", "x"], tmp_path, hits)
    flag = dict(zip(names, r.read_flags[1:]))
    assert [flag["q%d" % q] for q in (199, 200, 399, 400, 401)] == [0, 0, 0, 1, 1]
    assert [flag["q%d_at0" % q] for q in (199, 200, 399, 400, 401)] == [0, 0, 0, 1, 1]      # (the back never sees hit 0: it counts 399 there, and its 200th is still behind the front's)
    assert [flag["all%d" % n] for n in (1, 63, 64, 65, 1023, 1024, 1025)] == [0, 0, 0, 0, 1, 1, 1]
    assert r.mi[21][0] == r.mi[22][0] == trd.REF | trd.CORE and any(q[0] and not q[0] & trd.REF for q in r.mi)
    device_run(rs, ["-T", "1", "2000", "-rb", "1", "-rb", "3"], tmp_path, hits)
    trd.destroy(rs)


# ---- -T: one tested mod i = 1 and one partner m = 2 at the rules' thresholds ----

def ld_set(stem, visits, n, side="+", depth_m_extra=3, reverse=False, i_info=OK, m_info=OK):
    """`visits` reads hold i = 1; n of them hold m = 2 as well, behind it ("+"), before it ("-") or, one read each way, on both sides ("split");
    depth_m_extra reads hold m alone.  Mod 3 (no RDNA flag) fills; mod 4 is in no read: the reference sequence's only hit"""
    reads = []
    for v in range(visits):
        hits = [(3, True, 20), (1, not reverse, 40), (3, True, 30)]
        if v < n:
            before = (side == "-") != reverse if side != "split" else v % 2 == 0
            hits = [(2, True, 15)] + hits if before else hits + [(2, False, 25)]
        reads.append((500, hits))
    reads += [(300, [(2, True, 50)])] * depth_m_extra
    return trd.build_set(stem, K, W, 4, reads, [0, i_info, m_info, C1, C1])


LD_CASES = {      # name: (arguments of ld_set, run before the -T, expected [nGood, nMod2, nBadLD, nSplit] of i = 1 and nBadLD of m = 2)
    "2n==e": (dict(visits=10, n=5), 0, [0, 0, 0, 0], 0),
    "2n==e-1": (dict(visits=11, n=5), 0, [0, 1, 0, 0], 0),
    "n==0.8e": (dict(visits=10, n=8), 0, [1, 0, 0, 0], 0),
    "n==0.8e-1": (dict(visits=10, n=7, depth_m_extra=2), 0, [0, 0, 0, 0], 0),
    "n==depth[m]": (dict(visits=10, n=4, depth_m_extra=0), 0, [1, 0, 0, 0], 0),
    "n==1 cover 9 +": (dict(visits=9, n=1), 0, [0, 1, 0, 0], 0),
    "n==1 cover 10 +": (dict(visits=10, n=1), 0, [0, 1, 1, 0], 0),
    "n==1 cover 10 + all of m": (dict(visits=10, n=1, depth_m_extra=0), 0, [1, 0, 1, 0], 0),
    "n==1 cover 10 - all of m": (dict(visits=10, n=1, depth_m_extra=0, side="-"), 0, [1, 0, 0, 0], 1),
    "n==1 cover 9 - all of m": (dict(visits=9, n=1, depth_m_extra=0, side="-"), 0, [1, 0, 0, 0], 0),
    "- side reverse": (dict(visits=10, n=8, side="-", reverse=True), 0, [1, 0, 0, 0], 0),
    "split": (dict(visits=10, n=6, side="split"), 0, [0, 0, 0, 1], 0),
    "RUN 4 adds to m": (dict(visits=11, n=5), 3, [0, 1, 0, 0], 1),
    "one visit": (dict(visits=1, n=1, depth_m_extra=1), 0, [1, 0, 0, 0], 0),
}


@pytest.mark.parametrize("name", list(LD_CASES))
def test_ld_rules_at_their_thresholds(name, tmp_path):
    args, runs_before, want_i, want_bad_m = LD_CASES[name]
    rs = ld_set(str(tmp_path / "s"), **args)
    hits = (np.array([4], np.uint32), np.array([5], np.int32))
    device_run(rs, ["-R", "x"], tmp_path, hits)
    v = args["visits"]
    for _ in range(runs_before):                                      # the same call, for the RUN count; what it set to copy 0 is put back
        device_run(rs, ["-T", str(v), str(v + 1)], tmp_path, hits)
        rs.contents.ms.contents.info[1] = args.get("i_info", OK); rs.contents.ms.contents.info[2] = args.get("m_info", OK); mg.lib().mgModsetHostChanged(rs.contents.ms)
    r = device_run(rs, ["-T", str(v), str(v + 1)], tmp_path, hits)
    assert [r.mi[1][2], r.mi[1][3], r.mi[1][4], r.mi[1][5]] == want_i, r.mi[1]
    assert r.mi[2][4] == want_bad_m
    assert mg.readset_rdna_diag()[:3] == (1, 1, v)
    trd.destroy(rs)


def mixed_set(stem):
    """20 mods of every kind as tested mod and as partner: copy 0, REPEAT | RDNA, no RDNA flag, and good ones; i as the first and as the last hit of a read, i
    twice in a read, partners on one side and on both, reads on both strands, a read of 1300 hits"""
    rng = np.random.default_rng(11)
    info = [0] + [OK] * 20
    info[5] = RD                                  # copy 0
    info[6] = RD | trd.MS_REPEAT | C1
    info[7] = C1                                  # not RDNA
    info[8] = RD | 2; info[9] = RD | 3            # copy 2 and copy M pass
    reads = []
    for r in range(40):
        n = int(rng.integers(1, 30))
        mods = [int(m) for m in rng.integers(1, 21, n)]
        reads.append((int(rng.integers(0, 20)) + 20 * n + 30, [(m, bool(rng.integers(0, 2)), int(rng.integers(0, 20))) for m in mods]))
    reads.append((2000, [(1, True, 5)] + [(2, True, 9)] * 3 + [(1, False, 7)] + [(4, True, 3)]))      # i = 1 first, and again; i = 4 last
    reads.append((19000, [(int(m), True, 12) for m in rng.integers(1, 21, 1300)]))
    return trd.build_set(stem, K, W, 20, reads, info)


def test_every_kind_of_mod_in_batches(tmp_path):
    """the mixed set; depth equal to minDepth is tested and equal to maxDepth is not; MODGPU_TESTMODS_BATCH=3 crosses at least three batches (the diag
    call says so) and gives the same bytes as one batch"""
    rs = mixed_set(str(tmp_path / "m"))
    hits = (np.array([2, 3], np.uint32), np.array([10, 400], np.int32))
    r0 = trd.restatement_of(rs)
    depth = r0.depth
    lo, hi = sorted(set(depth[1:]))[1], sorted(set(depth[1:]))[-1]
    assert lo in depth and hi in depth
    after_r = device_run(rs, ["-R", "x"], tmp_path, hits)
    ok = [i for i in range(1, 21) if trd.check_mod(after_r.info[i])]
    assert 5 not in ok and 6 not in ok and 7 not in ok and 8 in ok and 9 in ok
    r = device_run(rs, ["-T", str(lo), str(hi)], tmp_path, hits)
    tested = r.diag[0]
    assert tested == sum(1 for i in ok if lo <= depth[i] < hi) and any(depth[i] == lo for i in ok) and tested >= 7
    assert mg.readset_rdna_diag() == (1,) + r.diag
    for i in (5, 6):
        assert r.mi[i][2:6] == [0, 0, 0, 0]
    trd.destroy(rs)
    rs = mixed_set(str(tmp_path / "m2"))
    with mg.knobs(TESTMODS_BATCH=3):
        device_run(rs, ["-R", "x"], tmp_path, hits)
        r2 = device_run(rs, ["-T", str(lo), str(hi)], tmp_path, hits)
    assert mg.readset_rdna_diag() == ((tested + 2) // 3,) + r.diag and (tested + 2) // 3 >= 3
    assert r2.zz == r.zz and r2.yy == r.yy and r2.mi == r.mi
    trd.destroy(rs)


def test_refusals_on_the_device(tmp_path):
    """with w > k: a visit with len - x - w < 0, and a distance beyond the count array; two tested mods whose count arrays pass the 20000 cells the
    reference clears between them; -1 and nothing modified"""
    hits = (np.array([1], np.uint32), np.array([7], np.int32))
    far = [(30000, [(1, True, 100), (2, True, 100)])] * 2
    rs = trd.build_set(str(tmp_path / "far"), K, W, 2, far, [0, OK, OK])
    mg.readset_ref_flag_hits(rs, *hits, None)
    with mg.knobs(READSET_HOST=0):
        with pytest.raises(mg.ModgpuError, match="20000"):
            mg.readset_test_mods(rs, 1, 100, None)
    assert mg.lib().mgReadsetRdnaPath() == -1 and mg.lib().mgReadsetTestModsRun(rs) == 0
    trd.destroy(rs)
    for reads, depth, rng_, what in (([(100, [(1, True, 10), (2, True, 75)])] * 3, None, (1, 100), "len - x - w"),
                                      ([(100, [(1, True, 5), (2, True, 75)]), (200, [(2, True, 50)])], None, (1, 2), "beyond")):
        rs = trd.build_set(str(tmp_path / what[:3]), 8, 30, 2, reads, [0, OK, OK], depth)
        mg.readset_ref_flag_hits(rs, *hits, None)
        before = (trd.mod_info_rows(rs), trd.ms_info(rs.contents.ms).tolist())
        with mg.knobs(READSET_HOST=0):
            with pytest.raises(mg.ModgpuError, match=what):
                mg.readset_test_mods(rs, rng_[0], rng_[1], None)
        assert mg.lib().mgReadsetRdnaPath() == -1 and (trd.mod_info_rows(rs), trd.ms_info(rs.contents.ms).tolist()) == before
        trd.destroy(rs)


# ---- randomized small sets ----

def random_set(stem, seed):
    rng = np.random.default_rng(seed)
    n_mods = int(rng.integers(3, 40))
    w = int(rng.integers(2, K + 1))                                   # w <= k
    info = [0] + [int(rng.choice([OK, OK, OK, RD | 2, C1, RD, RD | trd.MS_REPEAT | C1, 2])) for _ in range(n_mods)]
    reads = []
    for _ in range(int(rng.integers(1, 30))):
        n = int(rng.choice([0, 1, 2, 5, 20, 70, 130]))
        hits = [(int(rng.integers(1, n_mods + 1)), bool(rng.integers(0, 2)), int(rng.integers(0, 40))) for _ in range(n)]
        reads.append((sum(h[2] for h in hits) + K + int(rng.integers(0, 50)), hits))
    reads.append((300, [(1, True, 10), (2, False, 30), (1, True, 4)]))      # so that something is there to test
    info[1] = info[2] = OK
    return trd.build_set(stem, K, w, n_mods, reads, info), rng


@pytest.mark.parametrize("chunk", range(6))
def test_randomized_small_sets(chunk, tmp_path):
    """40 sets a chunk, w <= k and minDepth >= 1: -R from random hits, -T twice with -rb between, all on the device, against the restatement; none is a
    refusal and none is skipped"""
    done = 0
    for s in range(40):
        rs, rng = random_set(str(tmp_path / ("r%d" % s)), 1000 * chunk + s)
        n_mods = rs.contents.ms.contents.max
        hits = (rng.integers(1, n_mods + 1, 6).astype(np.uint32), rng.integers(0, 500, 6).astype(np.int32))
        depth = trd.restatement_of(rs).depth
        top = max(depth) + 1
        cmds = ["-R", "x", "-T", "1", str(top), "-rb", str(int(rng.integers(1, 4))), "-R", "x"]
        r = device_run(rs, cmds, tmp_path, hits)
        assert r.run_no == 1 and r.diag[0] >= 1
        done += 1
        trd.destroy(rs)
    assert done == 40


def test_example_runs_like_modasm(golden_dir, tmp_path):
    """examples/rdna_file.c = `modasm -r stem -R ref.fa -T 2 400 -T 2751 4751 -rb 2 -w out` on the library: the reference program's stdout, YY-TEST and
    ZZ-TEST files and, but for the addresses a file holds, its .mod and .readset bytes"""
    tag = list(trd.TAGS)[0]
    exe = str(tmp_path / "rdna_file")
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    r = subprocess.run(["gcc", "-O2", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "rdna_file.c"), "-o", exe,
                        "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    stem = trd.golden_stem(golden_dir, tag)
    g = trd.golden_out(golden_dir, tag, "example")
    out = str(tmp_path / "out")
    r = subprocess.run([exe, stem, stem + "_ref.fa", "2", "400", "2751", "4751", out], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-800:]
    assert r.stdout == g["stdout"] and "on the device" in r.stderr
    for n in ("1", "2"):
        assert open(str(tmp_path / ("YY-TEST" + n))).read() == g["YY"][n] and open(str(tmp_path / ("ZZ-TEST" + n))).read() == g["ZZ"][n]
    assert gzip.open(out + ".mod").read() == gzip.open(stem + "_X.mod").read()
    assert trs.readset_mask(gzip.open(out + ".readset").read()) == trs.readset_mask(gzip.open(stem + "_X.readset").read())


# ---- -T past one partner tile, share and scan step: the sets of tests/rdna_designs.py ----

def designed_run(name, tmp_path, want_z=True, batch=None):
    """a fresh load of the design through the device against its checked restatement; returns (restatement, Diag, Grid)"""
    from tests import rdna_designs as rd
    rs = rd.load(name, tmp_path)
    with mg.knobs(READSET_HOST=0, TESTMODS_BATCH=batch):
        out = rd.compare(name, rs, tmp_path, 0, want_z)
    trd.destroy(rs)
    return out


@pytest.mark.parametrize("want_z, batch", [(True, None), (False, None), (True, 1)])
def test_designed_three_partner_tiles(want_z, batch, tmp_path):
    """set A: nP = 8197, mgRdnaAccumKernel over blockIdx.y = 0 .. 2, the last tile of 5 ordinals; a tested mod with cells in tile 1 alone; one in tile 2
    that is its own partner; nSplitLD and nBadLD of other mods in tiles 1 and 2; with the ZZ lines (Emit over 33 steps of 256) and without; one batch
    and a batch per tested mod"""
    r, diag, grid = designed_run("A", tmp_path, want_z, batch)
    assert diag[0] == (3 if batch else 1)
    assert grid == (3, 16, 16, max(r.len) + 1)


@pytest.mark.parametrize("batch, share", [(1024, 1), (512, 2), (511, 4), (256, 4), (128, 8), (127, 16)])
def test_designed_visit_shares(batch, share, tmp_path):
    """set B: 1030 tested mods under MODGPU_TESTMODS_BATCH: the least share of the call is 1, 2, 4, 4, 8, 16 (mgRdnaAccumKernel's gridDim.z; with 1 a
    wave walks several visits), the last, smaller batch has 16; every call gives the restatement's YY, ZZ and ModInfo, so all give the same"""
    from tests import rdna_designs as rd
    assert (batch, share) in rd.B_BATCHES
    r, diag, grid = designed_run("B", tmp_path, True, batch)
    assert diag[0] == rd.batches_b(batch)
    assert grid == (1, share, 16, max(r.len) + 1)


@pytest.mark.parametrize("name", ["C", "D", "E513", "E256", "E257", "F"])
def test_designed_steps_of_256_and_64(name, tmp_path):
    """set C: 600 partners, a tested mod with cells on both sides of an empty step of 256 and one with every cell (mgRdnaRuleKernel's stride,
    mgRdnaEmitKernel's at += tot: the ZZ lines ascend in m); D: i's first occurrence at hits 0, 63, 64, 65, 127, 128, last, and twice in a read
    (mgRdnaVisitKernel); E: count arrays of exactly 513, 256 and 257 cells with the rules reading cells 0, 255, 256, 257, 512 (mgRdnaSuffixKernel's
    carry); F: dx = 65535 at hits 63, 64, 127 (mgRdnaPosKernel's carry)"""
    for want_z in (True, False):
        r, diag, grid = designed_run(name, tmp_path, want_z)
        assert diag[0] == 1
        assert grid == (1, 16, 16, max(r.len) + 1)
