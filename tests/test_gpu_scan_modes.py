"""GPU: the scan's six hit-test modes at every boundary of the choice between them, with proof of which instance ran.

mgScanKernel is twelve kernels -- MG_MODE_ANY / POW2 / FAST / ODD / ODD32 / ANY32 (csrc/mg_scan.hip), each with and without pos / read
-- and the iterator's kernel runs the six again.  The mode comes from (k, d) by four thresholds: dShift >= 3, B = shift1 + dShift <= 32,
k >= 17 (in effect 18: at k = 17 shift1 is 30 and B at least 33), and 2k <= 40 with the odd part of d below 2^15.  CASES below puts a
hasher ON each threshold and one step PAST it, and says beforehand which mode it must get: the table is written from the thresholds,
not read from the library.  mgScanDiag counts the launches where the template instance is chosen, and every leg asserts that the
instance it expected is the ONE that ran; then its output is held against the oracle.

Each case runs under no knob, under MODGPU_SCAN_DIV64=1 (ODD32 -> ODD, ANY32 -> ANY: the 64-bit test on the same input) and under
MODGPU_SCAN_GENERIC=1 (FAST -> POW2: the exact test on the same input), through three entry points: the batch scan with pos / read,
the batch scan of the k-mers alone with three workers (each owns hundreds of tiles and carries its candidate queue from tile to tile),
and the iterator's one-launch kernel.  The modset build runs each mode's k-mers-only kernel with the scan's digit counts on and off
and with the segments as the build's input and not."""
import functools

import numpy as np
import pytest

import modimizer_amd as mg
from oracle import pyoracle as po
import util
import test_gpu_modset as tm
import test_gpu_scan as ts

pytestmark = pytest.mark.gpu
TILE = ts.TILE
SEED = 17

#        (k, d, the mode the thresholds give)
CASES = [(17, 8, "POW2"),                                   # k = 17 can never be FAST: B = 30 + 3 = 33
         (18, 8, "FAST"), (18, 16, "FAST"),                 # the smallest FAST k (c2 = 4); (18, 16) has B = 32
         (18, 32, "POW2"),                                  # B = 33
         (19, 64, "FAST"), (19, 128, "POW2"),               # B = 32 / 33
         (21, 1024, "FAST"), (21, 2048, "POW2"),            # B = 32 / 33
         (31, 8, "FAST"), (31, 1 << 14, "FAST"),            # c2 = 30
         (24, 1 << 16, "FAST"), (31, 1 << 30, "FAST"),      # B = 32 with a large dShift: thresh = 2^16 and 4
         (20, 1 << 16, "POW2"),                             # B = 40
         (16, 4096, "POW2"),                                # k < 17
         (20, 3, "ODD32"), (20, 32767, "ODD32"),            # 40-bit hashes; the largest c24
         (21, 3, "ODD"), (21, 32767, "ODD"), (20, 32769, "ODD"),              # one step past each limit of the 32-bit test
         (20, 6, "ANY32"), (20, 24576, "ANY32"), (20, 65534, "ANY32"),        # dShift = 1, 13, 1 with odd part 3, 3, 32767
         (21, 6, "ANY"), (21, 24576, "ANY"), (20, 65538, "ANY")]              # one step past
KNOBS = [None, "SCAN_DIV64", "SCAN_GENERIC"]
BUILD_CASES = [(21, 64, 22, "FAST"), (31, 4, 24, "POW2"), (19, 31, 22, "ODD32"), (31, 97, 22, "ODD"), (17, 1000, 22, "ANY32"), (21, 96, 22, "ANY")]


def mode_under(mode, knob):
    """what the knob makes of the mode: SCAN_DIV64 takes the 32-bit tests away, SCAN_GENERIC the filter, and neither touches the rest"""
    if knob == "SCAN_DIV64":
        return {"ODD32": "ODD", "ANY32": "ANY"}.get(mode, mode)
    if knob == "SCAN_GENERIC":
        return {"FAST": "POW2"}.get(mode, mode)
    return mode


def scan_knobs(knob, **more):
    kv = dict(SCAN_DIV64=None, SCAN_GENERIC=None, SCAN_GRID=None, SCAN_HIST=None, NO_SEGMENT_INPUT=None)
    if knob:
        kv[knob] = 1
    kv.update(more)
    return mg.knobs(**kv)


def test_the_table_follows_the_thresholds():
    """CASES against the four thresholds as the module's first lines state them (no library in it), and every mode and both sides of every
    threshold are there"""
    for k, d, mode in CASES:
        shift = (d & -d).bit_length() - 1
        odd = d >> shift
        if odd == 1:
            want = "FAST" if shift >= 3 and (64 - 2 * k) + shift <= 32 and k >= 17 else "POW2"
        else:
            small = 2 * k <= 40 and odd < (1 << 15)
            want = ("ODD32" if small else "ODD") if shift == 0 else ("ANY32" if small else "ANY")
        assert mode == want, (k, d)
    assert {m for _, _, m in CASES} == set(util.SCAN_MODES)


# ---- inputs: made once per (k, d), shared by the knob legs ---------------------------------------------------------------------------

def kmer_bases(x, k):
    return np.array([(x >> (2 * (k - 1 - i))) & 3 for i in range(k)], np.uint8)


def kmer_revcomp(x, k):
    r = 0
    for i in range(k):
        r |= (3 - ((x >> (2 * i)) & 3)) << (2 * (k - 1 - i))
    return r


def planted_read(oh, k, d, rng, n=200):
    """a read of n k-mers whose FORWARD hash is 0 modulo the power of two d, every other one as its reverse complement (so both strands
    hit), three random bases between them.  hash = (kmer * f1 mod 2^64) >> shift1: with B = shift1 + log2 d <= 2k and f1 odd, low B bits
    of y / f1 mod 2^B for a y < 2^shift1 make bits [shift1, B) of the product zero, whatever the bits above.  About half of them are
    modimizers -- the others lose to their other strand, whose hash is smaller: the oracle says which"""
    shift1 = 64 - 2 * k
    B = shift1 + d.bit_length() - 1
    assert d & (d - 1) == 0 and B <= 2 * k
    f1 = int(oh.c.factor1)
    inv = pow(f1, -1, 1 << B)
    parts = []
    for i in range(n):
        y = int(rng.integers(0, 1 << shift1))
        x = ((int(rng.integers(0, 1 << 62)) << B) | ((y * inv) & ((1 << B) - 1))) & ((1 << (2 * k)) - 1)
        assert (((x * f1) & ((1 << 64) - 1)) >> shift1) % d == 0
        parts += [kmer_bases(kmer_revcomp(x, k) if i & 1 else x, k), rng.integers(0, 4, 3).astype(np.uint8)]
    return np.concatenate(parts)


@functools.lru_cache(maxsize=3)
def case_inputs(k, d):
    """the batch of a case, its iterator reads, and the oracle's answers to both"""
    oh = po.Hasher(k, d, SEED)
    rng = np.random.default_rng(SEED)
    big = rng.integers(0, 4, 4_000_000).astype(np.uint8)          # d up to 65538 still has hits
    planted = planted_read(oh, k, d, rng) if d & (d - 1) == 0 and d >= (1 << 14) else None     # natural hits are too rare there
    src = planted if planted is not None else big
    _, pos, _ = oh.scan(src)
    assert len(pos), (k, d)
    dense = np.tile(src[pos[0]:pos[0] + k], 300)                  # a hit every k bases: fills the candidate list, overflows a worker's segment
    lens = [TILE - k + 1, k - 1, TILE, 1, TILE - 1, 2, TILE + k - 1, TILE - 20, 20, 21, 22, 3 * TILE + 5, 19, TILE // 2, TILE // 2,
            TILE + 1, TILE - 1, TILE + k, TILE + k - 2, 2 * TILE - k, 2 * TILE + k - 1, k, TILE - k, TILE - k - 1, TILE - k + 2]     # test_tile_boundaries'
    reads = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    reads += [np.zeros(0, np.uint8), dense, np.zeros(0, np.uint8), rng.integers(0, 4, k - 1).astype(np.uint8), big]
    if planted is not None:
        reads += [planted, rng.integers(0, 4, 5).astype(np.uint8)]
    bases, offs = util.concat_reads(reads)
    want = util.oracle_scan_batch(oh, bases, offs)
    # what keeps the case from being vacuous, on the oracle's output alone
    ek, _, ef, _ = want
    counts = (len(ek), int((ef == 1).sum()), int((ef == 0).sum()))
    print("case (%d, %d): %d oracle hits, %d forward, %d reverse" % ((k, d) + counts))
    assert counts[0] >= 16 and counts[1] >= 4 and counts[2] >= 4, (k, d, counts)
    iter_reads = [dense, big[:64 * TILE]] + ([planted] if planted is not None else [])
    return bases, offs, want, [(r, oh.scan(r)) for r in iter_reads]


def only(since, key):
    assert set(since) == {key} and since[key] >= 1, (since, key)


def scan_kmers_only(sh, bases, offs, n_expected):
    """seqhashScanBatchDevice with dPosF and dReadId both NULL (the build's kernel), a second time with the capacity it names if a worker's
    segment ran over: the k-mers"""
    L = mg.lib()
    total, n_reads = len(bases), len(offs) - 1
    d_packed = mg.DeviceBuffer.from_numpy(mg.pack_host(bases))
    d_off = mg.DeviceBuffer.from_numpy(offs.astype(np.uint64))
    d_cnt = mg.DeviceBuffer(32)
    cap = n_expected + n_expected // 4 + 1024
    for attempt in range(2):
        d_work = mg.DeviceBuffer(L.mgScanWorkBytes(total, n_reads, cap))
        d_k = mg.DeviceBuffer(cap * 8)
        mg.check(L.seqhashScanBatchDevice(sh, d_packed.ptr, total, d_off.ptr, n_reads, d_k.ptr, None, None, cap, d_cnt.ptr, d_work.ptr, None))
        cnt = d_cnt.to_numpy(np.uint64, 4)
        assert int(cnt[0]) == n_expected
        if not cnt[1]:
            return d_k.to_numpy(np.uint64, n_expected)
        assert attempt == 0 and int(cnt[3]) >= n_expected
        cap = int(cnt[3])


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("k,d,mode", CASES)
def test_mode_boundaries(k, d, mode, knob):
    bases, offs, (ek, ep, ef, est), iter_reads = case_inputs(k, d)
    ran = mode_under(mode, knob)
    sh = mg.seqhashCreate(k, d, SEED)
    with scan_knobs(knob):
        # the batch scan with pos / read
        before = util.scan_diag()
        km, pos, isf, st = mg.scan_batch(sh, bases, offs)
        only(util.scan_diag_since(before), ("batch", ran, 1))
        assert np.array_equal(st, est) and np.array_equal(km, ek) and np.array_equal(pos, ep) and np.array_equal(isf, ef)
        # the iterator's kernel (crossover 0), reads of at most 64 tiles
        for read, (ik, ip, if_) in iter_reads:
            before = util.scan_diag()
            a, p, f = ts._iterate_arrays(sh, read)
            only(util.scan_diag_since(before), ("iter", ran))
            assert np.array_equal(a, ik) and np.array_equal(p, ip) and np.array_equal(f, if_), len(read)
    # the k-mers alone, three workers: every worker owns hundreds of tiles and its candidate queue goes from tile to tile
    with scan_knobs(knob, SCAN_GRID=3):
        before = util.scan_diag()
        km = scan_kmers_only(sh, bases, offs, len(ek))
        only(util.scan_diag_since(before), ("batch", ran, 0))
        assert np.array_equal(km, ek)


# ---- the modset build: each mode's k-mers-only kernel feeding the table --------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def build_inputs(k, d, bits):
    batch = tm.synth_batch(600_000 if d > 4 else 150_000, 50_000, 11)
    oms, total = tm.oracle_build(po.Hasher(k, d, SEED), bits, [batch])
    return batch, oms, total


@pytest.mark.parametrize("leg", [{}, {"SCAN_HIST": 0}, {"NO_SEGMENT_INPUT": 1}], ids=["hist", "hist0", "dense"])
@pytest.mark.parametrize("k,d,bits,mode", BUILD_CASES)
def test_build_per_mode(k, d, bits, mode, leg):
    """mgAddSequenceBatch against the oracle's set (values, depths, index table) by the bucketed build, which takes the scan's segments and
    its count of the first digit: with the scan counting, with the compaction kernel counting, and with a dense copy as the build's input"""
    batch, oms, total = build_inputs(k, d, bits)
    sh = mg.seqhashCreate(k, d, SEED)
    with scan_knobs(None, TABLE_PATH="bucket", **leg):
        ms = mg.modsetCreate(sh, bits)
        before = util.scan_diag()
        n = mg.add_sequence_batch(ms, *batch)
        only(util.scan_diag_since(before), ("batch", mode, 0))
        assert n == total
        tm.assert_same_modset(ms, oms, bits)
        mg.lib().modsetDestroy(ms)
