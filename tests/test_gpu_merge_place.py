"""GPU: the merge kernel's placement by prefix scan (MODGPU_MERGE_PLACE=1: a bucket that is empty before the add is laid out
from its keys' home counts, one prefix sum and one prefix max, without a probe -- csrc/mg_bucket.hip mgPlaceStarts).  The table's
slot order is not part of any parity contract; value[] / depth[] / index[] and every lookup's answer are, and the layout itself is
checked by mgTableCheckLayout, which walks the device table without going through the lookups."""
import ctypes as C

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import synth
from oracle import pyoracle as po
import util

pytestmark = pytest.mark.gpu


def synth_batch(total, genome_bases, seed, err=0.03, n50=4000):
    genome = synth.iid_bases(genome_bases, seed)
    starts, offs, strands = synth.ont_read_plan(total, genome_bases, seed + 1, n50=n50, lo=30, hi=30000)
    return synth.reads_from_genome(genome, starts, offs, strands, err, seed + 2), offs.astype(np.int64)


def oracle_build(oh, bits, batches):
    oms = po.Modset(oh, bits)
    for bases, offs in batches:
        for r in range(len(offs) - 1):
            oms.add_sequence(bases[offs[r]:offs[r + 1]])
    return oms


def layout(ms):
    """(broken paths, keys in a wrong bucket, duplicates, keys, buckets laid out by scan, those that ran over their end)"""
    out = (C.c_uint64 * 6)()
    mg.check(mg.lib().mgTableCheckLayout(ms, out))
    return [int(x) for x in out]


def assert_same_modset(ms, oms, bits):
    mg.check(mg.lib().modsetSyncToHost(ms, 1))
    assert ms.contents.max == oms.max
    v, d, _ = mg.modset_arrays(ms)
    assert np.array_equal(v[1:], oms.values()[1:]), "values"
    assert np.array_equal(d[1:], oms.depths()[1:]), "depths"
    assert np.array_equal(np.ctypeslib.as_array(ms.contents.index, (1 << bits,)), oms.index_table()), "index[]"


def device_find(ms, kmers):
    L = mg.lib()
    d_p = mg.DeviceBuffer.from_numpy(kmers); d_o = mg.DeviceBuffer(len(kmers) * 4)
    mg.check(L.modsetFindBatchDevice(ms, d_p.ptr, len(kmers), d_o.ptr, None))
    return d_o.to_numpy(np.uint32, len(kmers))


K, W, BITS = 21, 16, 22


@pytest.mark.parametrize("knobs", [{"TIGHT_LOAD": 50}, {"TIGHT_LOAD": 70}, {"TIGHT_LOAD": 85},
                                   {"BUCKET_R": 256, "BUCKET_T": 256, "TABLE_LOAD": 85, "TIGHT_LOAD": 0}])
def test_layout_is_sound(knobs):
    """the table the scan lays out is an ordinary linear-probing table at every load, also where a bucket's entries run over its
    end and come in again at slot 0 (small buckets at load 0.85: the last case must really see that happen)"""
    sh = mg.seqhashCreate(K, W, 17); oh = po.Hasher(K, W, 17)
    b = synth_batch(1_500_000, 400_000, 41)
    with mg.knobs(MERGE_PLACE=1, TABLE_PATH="bucket", **knobs):
        ms = mg.modsetCreate(sh, BITS)
        mg.add_sequence_batch(ms, *b)
        lay = layout(ms)
        print("knobs", knobs, "layout", lay, "slots", mg.lib().mgModsetDeviceSlots(ms))
        assert lay[:3] == [0, 0, 0] and lay[3] == ms.contents.max
        assert lay[4] > 0, "no bucket went through the scan placement"
        if "BUCKET_R" in knobs:
            assert lay[5] > 0, "no bucket ran over its end: the wrap was not exercised"
        assert_same_modset(ms, oracle_build(oh, BITS, [b]), BITS)
        mg.lib().modsetDestroy(ms)


def test_same_results_as_the_claims():
    """MODGPU_MERGE_PLACE=0 and =1 on the same input: identical value[], depth[], max and identical answers from modsetIndexFind
    for every inserted k-mer and as many absent ones"""
    L = mg.lib()
    sh = mg.seqhashCreate(K, W, 17); oh = po.Hasher(K, W, 17)
    b = synth_batch(2_400_000, 700_000, 43)
    km = np.unique(util.oracle_scan_batch(oh, *b)[0])
    rng = np.random.default_rng(5)
    absent = np.setdiff1d(rng.integers(0, 1 << (2 * K), len(km) + 1000).astype(np.uint64), km)[:len(km)]
    res = []
    for place in (0, 1):
        # TABLE_LOAD=80 also for the lookups: they would otherwise bring the table to load 0.4 first, by a rehash that claims
        with mg.knobs(MERGE_PLACE=place, TABLE_PATH="bucket", TIGHT_LOAD=70, TABLE_LOAD=80):
            ms = mg.modsetCreate(sh, BITS)
            mg.add_sequence_batch(ms, *b)
            slots = L.mgModsetDeviceSlots(ms)
            dev = device_find(ms, np.concatenate([km, absent]))
            assert L.mgModsetDeviceSlots(ms) == slots and slots > 1 << 16, "the lookups must see the table as it was built"
            mg.check(L.modsetSyncToHost(ms, 1))
            v, d, _ = mg.modset_arrays(ms)
            host = np.array([L.modsetIndexFind(ms, int(x), 0) for x in np.concatenate([km, absent])], np.uint32)
            res.append((int(ms.contents.max), v.copy(), d.copy(), host, dev, layout(ms)))
            L.modsetDestroy(ms)
    (m0, v0, d0, h0, f0, l0), (m1, v1, d1, h1, f1, l1) = res
    assert l0[4] == 0 and l1[4] > 0, (l0, l1)
    assert m0 == m1 and np.array_equal(v0[1:], v1[1:]) and np.array_equal(d0[1:], d1[1:])         # (entry 0 is not an entry: modset.h)
    assert np.array_equal(h0, h1) and np.array_equal(f0, f1) and np.array_equal(h1, f1)
    assert (h1[:len(km)] != 0).all() and (h1[len(km):] == 0).all()


def test_later_batches_on_a_placed_table():
    """a second and a third batch into the set the scan built: the dedup kernel loads the image and claims into it, the merge
    kernel takes its old paths for every bucket that holds entries"""
    sh = mg.seqhashCreate(K, W, 17); oh = po.Hasher(K, W, 17)
    b1 = synth_batch(600_000, 60_000, 11)
    b2 = synth_batch(300_000, 60_000, 11, err=0.05)
    b3 = synth_batch(300_000, 90_000, 13)
    for slots in (None, 0, 1):
        with mg.knobs(MERGE_PLACE=1, TABLE_PATH="bucket", MERGE_SLOTS=slots):
            ms = mg.modsetCreate(sh, BITS)
            for b in (b1, b2, b3):
                mg.add_sequence_batch(ms, *b)
            lay = layout(ms)
            assert lay[:3] == [0, 0, 0] and lay[3] == ms.contents.max and lay[4] > 0, lay
            assert_same_modset(ms, oracle_build(oh, BITS, [b1, b2, b3]), BITS)
            mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("slots", [1, 0, None])
def test_empty_buckets_of_a_filled_table(slots):
    """a tiny first batch leaves most buckets of the table empty; a large second batch then meets empty buckets in a table that is
    not empty -- with carried slots (MODGPU_MERGE_SLOTS=1: a list entry holds its slot above the k-mer, and goes where it says) and
    without (the scan) -- and a third batch, the second again, must find every k-mer there: no new entry"""
    sh = mg.seqhashCreate(K, W, 17); oh = po.Hasher(K, W, 17)
    b1 = util.concat_reads([synth.iid_bases(150, 51)])              # a handful of k-mers: they cannot fill every bucket
    b2 = synth_batch(1_500_000, 400_000, 53)
    with mg.knobs(MERGE_PLACE=1, TABLE_PATH="bucket", MERGE_SLOTS=slots):
        ms = mg.modsetCreate(sh, BITS)
        mg.add_sequence_batch(ms, *b1)
        placed1 = layout(ms)[4]
        assert 0 < ms.contents.max < 16
        mg.add_sequence_batch(ms, *b2)
        max2 = ms.contents.max
        lay = layout(ms)
        print("slots", slots, "placed by the first add", placed1, "layout after the second", lay)
        assert lay[:3] == [0, 0, 0] and lay[3] == max2, lay
        if slots == 0:
            assert lay[4] > placed1, "the second add met no empty bucket: the case is not exercised"
        mg.add_sequence_batch(ms, *b2)
        assert ms.contents.max == max2, "k-mers of the second batch were not found again"
        lay3 = layout(ms)
        assert lay3[:4] == lay[:4], (lay, lay3)
        assert_same_modset(ms, oracle_build(oh, BITS, [b1, b2, b2]), BITS)
        mg.lib().modsetDestroy(ms)


DIAG, diag = util.DIAG, util.table_diag          # mgTableDiag: the table's geometry and the launches by kernel since it was made


@pytest.mark.parametrize("find8", [0, 1])
@pytest.mark.parametrize("path", ["direct", "part", "2"])
def test_lookups_on_a_placed_table(path, find8):
    """direct probes, the partitioned lookups and the two-level ones over the 16-byte slots and over the 8-byte copy, on a table the
    scan laid out.  Only the scan-fed query (mgQueryReadsDevice) takes the partitioned paths, and two levels need more than 512
    buckets: 1024 x 192 slots here (MODGPU_BUCKET_R=256), 2k - log2 NB = 32.  mgTableDiag says which kernel ran."""
    sh = mg.seqhashCreate(K, W, 17); oh = po.Hasher(K, W, 17)
    L = mg.lib()
    b = synth_batch(3_000_000, 900_000, 47)
    q = synth_batch(600_000, 900_000, 47, err=0.08)
    qk = util.oracle_scan_batch(oh, *q)[0]
    oms = oracle_build(oh, BITS, [b])
    want = np.array([oms.find(x) for x in qk], np.uint32)
    # a lookup batch first brings the table to its own load (0.4, by a rehash that places with claims) unless the table is sparse enough
    # already: TABLE_LOAD=100 holds for the lookups too, the table is past the 2^16-slot floor, and the slot count and the counter of
    # scan-placed buckets must be what the build left -- the lookups then run on the layout the scan made
    with mg.knobs(MERGE_PLACE=1, TABLE_PATH="bucket", TIGHT_LOAD=80, TABLE_LOAD=100, BUCKET_R=256, BUCKET_T=256):
        ms = mg.modsetCreate(sh, BITS)
        mg.add_sequence_batch(ms, *b)
        slots = L.mgModsetDeviceSlots(ms)
        lay = layout(ms)
        assert lay[:3] == [0, 0, 0] and lay[4] > 0 and slots > 1 << 16 and lay[3] * 100 > slots * 60, (lay, slots)
        d0 = diag(ms)
        assert d0["log2NB"] == 10 and 2 * K - d0["log2NB"] == 32, d0
        d_p = mg.DeviceBuffer.from_numpy(mg.pack_host(q[0])); d_o = mg.DeviceBuffer.from_numpy(q[1].astype(np.uint64))
        d_ix = mg.DeviceBuffer((len(qk) + 8) * 4)
        n = C.c_uint64()
        with mg.knobs(FIND_PATH=path, FIND8=find8):
            mg.check(L.mgQueryReadsDevice(ms, d_p.ptr, int(q[1][-1]), d_o.ptr, len(q[1]) - 1, d_ix.ptr, None, None, len(qk) + 8, C.byref(n), None))
            assert n.value == len(qk)
            got = d_ix.to_numpy(np.uint32, len(qk))
            d1 = diag(ms)
            also = device_find(ms, qk)                    # (modsetFindBatchDevice: direct probes whatever the knobs say)
        ran = {c for c in DIAG[2:6] if d1[c] != d0[c]}
        assert ran == {{"direct": "direct", "part": "part1", "2": "part2_8" if find8 else "part2_16"}[path]}, (path, find8, d0, d1)
        assert d1["pack8"] - d0["pack8"] == (1 if (path, find8) == ("2", 1) else 0)
        assert L.mgModsetDeviceSlots(ms) == slots, "the lookups rehashed the table: they did not see the scan's layout"
        assert layout(ms) == lay
        assert np.array_equal(got, want) and (got == 0).any() and (got != 0).any()
        assert np.array_equal(also, want)
        mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("extra", [-1, 0])
def test_full_bucket(extra):
    """a bucket offered R - 1 keys takes them all (no empty slot left but one); offered R it raises the overflow flag -- the add
    fails with MG_ERR_CAPACITY -- and nothing is written outside the bucket"""
    L = mg.lib()
    R = 256
    rng = np.random.default_rng(9)
    sh = mg.seqhashCreate(21, 64, 17)
    base = util.kmers_with_mix_prefix(rng, 20_000, 1, 1, 21)           # the table hash starts with a one bit: a bucket of the upper half
    hot = util.kmers_with_mix_prefix(rng, R + extra, 0, 10, 21)          # ... with ten zero bits: bucket 0 of any table of up to 1024 buckets
    with mg.knobs(MERGE_PLACE=1, TABLE_PATH="bucket", BUCKET_R=R, BUCKET_T=256, TIGHT_LOAD=0, MERGE_SLOTS=0):
        ms = mg.modsetCreate(sh, 20)
        d_b = mg.DeviceBuffer.from_numpy(base)
        mg.check(L.modsetAddBatchDevice(ms, d_b.ptr, len(base), None, 1, None))
        slots = L.mgModsetDeviceSlots(ms)
        assert slots % R == 0 and 2 <= slots // R <= 1024, slots                # bucket 0 is the k-mers' of `hot`, and is empty
        lay0 = layout(ms)
        assert lay0[:3] == [0, 0, 0] and lay0[3] == len(base)
        d_h = mg.DeviceBuffer.from_numpy(hot)
        st = L.modsetAddBatchDevice(ms, d_h.ptr, len(hot), None, 1, None)
        lay = layout(ms)
        print("extra", extra, "status", st, "layout before", lay0, "after", lay)
        assert L.mgModsetDeviceSlots(ms) == slots
        assert lay[1] == 0 and lay[2] == 0, "a key outside its bucket"
        if extra < 0:
            assert st == 0 and lay[0] == 0 and lay[3] == len(base) + len(hot) and lay[4] == lay0[4] + 1
            got = device_find(ms, np.concatenate([hot, base[:1000]]))
            assert (got[:len(hot)] == np.arange(len(base) + 1, len(base) + len(hot) + 1)).all() and (got[len(hot):] != 0).all()
        else:
            assert st == 4, st                                                  # MG_ERR_CAPACITY
            assert lay[0] == 0 and lay[3] == len(base), "the refused bucket must stay empty, the others as they were"
        L.modsetDestroy(ms)


def test_hot_buckets():
    """poly-A and a satellite repeat (tests/skew_probe.py's kind): buckets with a k-mer of very many copies, with the scan on"""
    k, w, bits = 21, 1, 22
    sh = mg.seqhashCreate(k, w, 17); oh = po.Hasher(k, w, 17)
    rng = np.random.default_rng(3)
    monomer = rng.integers(0, 4, 171).astype(np.uint8)
    reads = [np.zeros(300_000, np.uint8), rng.integers(0, 4, 200_000).astype(np.uint8), np.full(100_000, 3, np.uint8),
             np.tile(monomer, 1500), rng.integers(0, 4, 150_000).astype(np.uint8)]
    b = util.concat_reads(reads)
    for knobs in ({}, {"HOT_SPLIT": "200,64"}, {"TIGHT_LOAD": 80}):
        with mg.knobs(MERGE_PLACE=1, TABLE_PATH="bucket", **knobs):
            ms = mg.modsetCreate(sh, bits)
            mg.add_sequence_batch(ms, *b)
            lay = layout(ms)
            assert lay[:3] == [0, 0, 0] and lay[3] == ms.contents.max and lay[4] > 0, (knobs, lay)
            assert_same_modset(ms, oracle_build(oh, bits, [b]), bits)
            mg.lib().modsetDestroy(ms)
