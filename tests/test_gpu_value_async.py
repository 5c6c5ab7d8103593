"""GPU: the bucketed add's value writer off the caller's stream (MODGPU_VALUE_ASYNC; csrc/mg_rank.hip mgValueWriteKernel, csrc/mg_modsetdev.hip
mgValueSettle).  The add's rank records go out on the caller's stream, value[] is written behind the merge kernel on a stream of the set's own and
may still be on its way when the call returns: every reader of value[] and everything that frees or reuses what the writer reads has to wait for
it, the next add's scan has to go into the other scratch arena.  Every case runs with the writer forced onto that stream (1) and kept on the
caller's (0), both against the oracle on value[], depth[], index[] and max; mgValueWriterDiag proves which of the two ran."""
import ctypes as C
import threading

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import synth
from oracle import pyoracle as po
import util
from test_gpu_merge_place import assert_same_modset, device_find, oracle_build, synth_batch

pytestmark = pytest.mark.gpu

K, W, BITS = 21, 16, 22
MG_ERR_CAPACITY = 4
RANK_UNITS = 8192                     # MG_RANK_UNITS of csrc/mg_rank.hip: the waves that share the ordered flag count
MODES = [1, 0]


def knobs(va, **more):
    return mg.knobs(VALUE_ASYNC=va, TABLE_PATH="bucket", **more)


class DevReads:
    """a batch of reads packed and on the device, as mgAddReadsDevice takes it"""

    def __init__(self, batch):
        bases, offs = batch
        self.total, self.n_reads = int(offs[-1]), len(offs) - 1
        self.d_p = mg.DeviceBuffer.from_numpy(mg.pack_host(bases))
        self.d_o = mg.DeviceBuffer.from_numpy(offs.astype(np.uint64))

    def add(self, ms):
        """(status, modimizers)"""
        n = C.c_uint64()
        st = mg.lib().mgAddReadsDevice(ms, self.d_p.ptr, self.total, self.d_o.ptr, self.n_reads, C.byref(n), None)
        return st, n.value


def add_ok(ms, dr):
    st, n = dr.add(ms)
    mg.check(st)
    return n


def writers():
    """mgValueWriterDiag: (launches off the caller's stream, launches on it) since the process started"""
    out = (C.c_uint64 * 2)()
    mg.check(mg.lib().mgValueWriterDiag(out))
    return np.array([int(out[0]), int(out[1])])


def ran(va, launches=1):
    """what `launches` bucketed adds under MODGPU_VALUE_ASYNC=va add to writers ()"""
    return [launches, 0] if va == 1 else [0, launches]


@pytest.fixture(scope="module")
def hashers():
    return mg.seqhashCreate(K, W, 17), po.Hasher(K, W, 17)


@pytest.fixture(scope="module")
def shared(hashers):
    """one batch of test_gpu_merge_place.py's size, its modimizers and the oracle's set of it: built once, only read"""
    _, oh = hashers
    b = synth_batch(1_500_000, 400_000, 61)
    km = util.oracle_scan_batch(oh, *b)[0]
    return b, km, oracle_build(oh, BITS, [b])


@pytest.mark.parametrize("va", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_row_boundaries(va, n):
    """1, 63, 64 and 65 modimizers: less than a row of 64 ordinals, a row less one, a whole row, a row and one"""
    sh = mg.seqhashCreate(K, 1, 17); oh = po.Hasher(K, 1, 17)         # w = 1: a read of k bases is one modimizer
    rng = np.random.default_rng(100 + n)
    kept, bases, offs = util.kmer_reads(oh, rng.integers(0, 1 << (2 * K), 4 * n + 16).astype(np.uint64), K)
    assert len(kept) >= n
    b = (bases[:n * K], offs[:n + 1])
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS)
        w0 = writers()
        assert add_ok(ms, DevReads(b)) == n
        assert (writers() - w0).tolist() == ran(va)
        assert_same_modset(ms, oracle_build(oh, BITS, [b]), BITS)
        mg.lib().modsetDestroy(ms)


@pytest.fixture(scope="module")
def big(hashers):
    _, oh = hashers
    b = synth_batch(12_000_000, 1_500_000, 67, err=0.01)
    return b, oracle_build(oh, BITS, [b])


@pytest.mark.parametrize("va", MODES)
def test_above_one_rank_unit(va, hashers, big):
    """more rows than rank units (every unit walks more than one row, the writer's waves more than one step) and a partial last row"""
    sh, _ = hashers
    b, oms = big
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS)
        n = add_ok(ms, DevReads(b))
        print("modimizers", n, "rows", (n + 63) // 64, "entries", oms.max)
        assert n > RANK_UNITS * 64 and n % 64 != 0
        assert_same_modset(ms, oms, BITS)
        mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("va", MODES)
def test_repeated_adds(va, hashers):
    """three adds in a row, nothing between them, then one sync.  The second shares k-mers with the first; the sizes differ, so a scratch
    arena has to grow while a write is pending"""
    sh, oh = hashers
    bs = [synth_batch(300_000, 120_000, 71), synth_batch(1_500_000, 120_000, 71, err=0.05), synth_batch(600_000, 200_000, 73)]
    drs = [DevReads(b) for b in bs]
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS)
        w0 = writers()
        for dr in drs:
            add_ok(ms, dr)
        assert (writers() - w0).tolist() == ran(va, 3)
        assert_same_modset(ms, oracle_build(oh, BITS, bs), BITS)
        mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("va", MODES)
def test_clear_between_adds(va, hashers):
    """add A, clear (which does not wait), add B: the set is B's alone, A's writer has not landed on B's values"""
    sh, oh = hashers
    a, b = synth_batch(1_500_000, 400_000, 75), synth_batch(700_000, 300_000, 77)
    da, db = DevReads(a), DevReads(b)
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS)
        add_ok(ms, da)
        mg.check(mg.lib().mgModsetClear(ms, None))
        add_ok(ms, db)
        assert_same_modset(ms, oracle_build(oh, BITS, [b]), BITS)
        mg.lib().modsetDestroy(ms)


@pytest.fixture(scope="module")
def large_then_small():
    """(hasher, table bits, a batch of more than 1.5e6 modimizers, a small one, the oracle's set of the small one alone)"""
    k, w, bits = 21, 8, 23
    a, b = synth_batch(14_000_000, 1_500_000, 91, err=0.01), synth_batch(400_000, 150_000, 93)
    return mg.seqhashCreate(k, w, 17), bits, a, b, oracle_build(po.Hasher(k, w, 17), bits, [b])


@pytest.mark.parametrize("va", [None, 1, 0])
def test_clear_then_direct_add(va, large_then_small):
    """under the library's own choice of leg: a batch of more than 1.5e6 modimizers goes by buckets and (knob unset or 1) leaves its writer
    running; the set is cleared, which does not wait; a small batch then goes by the direct leg, whose kernel writes value[1 ..] on the caller's
    stream.  That stream has to wait for the first add's writer, which stores to the same entries: the set is the small batch's alone"""
    sh, bits, a, b, ob = large_then_small
    da, db = DevReads(a), DevReads(b)
    with mg.knobs(VALUE_ASYNC=va):
        ms = mg.modsetCreate(sh, bits)
        w0 = writers()
        na = add_ok(ms, da)
        w1 = writers()
        mg.check(mg.lib().mgModsetClear(ms, None))
        nb = add_ok(ms, db)
        w2 = writers()
        print("modimizers", na, nb, "writers", (w1 - w0).tolist(), (w2 - w1).tolist())
        assert na > 1_500_000 and nb < 1_500_000
        assert (w1 - w0).tolist() == ran(0 if va == 0 else 1), "the large batch did not go by buckets"
        assert (w2 - w1).tolist() == [0, 0], "the small batch did not go by the direct leg"
        assert_same_modset(ms, ob, bits)
        mg.lib().modsetDestroy(ms)


def read_find(ms, b, km, oms):
    want = np.array([oms.find(x) for x in km[:20000]], np.uint32)
    assert np.array_equal(device_find(ms, km[:20000]), want) and (want != 0).all()


def read_query(ms, b, km, oms):
    L = mg.lib()
    q = (b[0][:int(b[1][40])], b[1][:41])                                   # the batch's first 40 reads
    d_p = mg.DeviceBuffer.from_numpy(mg.pack_host(q[0])); d_o = mg.DeviceBuffer.from_numpy(q[1].astype(np.uint64))
    cap = len(q[0]) // W * 2 + 64
    d_ix = mg.DeviceBuffer(cap * 4); n = C.c_uint64()
    mg.check(L.mgQueryReadsDevice(ms, d_p.ptr, int(q[1][-1]), d_o.ptr, 40, d_ix.ptr, None, None, cap, C.byref(n), None))
    assert 0 < n.value <= cap
    want = np.array([oms.find(x) for x in km[:n.value]], np.uint32)
    assert np.array_equal(d_ix.to_numpy(np.uint32, n.value), want) and (want != 0).all()


def read_hist(ms, b, km, oms):
    d_h = mg.DeviceBuffer.from_numpy(np.zeros(65536, np.uint64))
    mg.check(mg.lib().modsetDepthHistogramDevice(ms, d_h.ptr, None))
    mg.check(mg.lib().mgStreamSynchronize(None))
    assert np.array_equal(d_h.to_numpy(np.uint64, 65536)[1:], np.bincount(oms.depths()[1:], minlength=65536).astype(np.uint64)[1:])


def read_view(ms, b, km, oms):
    view = mg.lib().mgHookDeviceView                                        # (what a sender of a rank-order merge and the reports call)
    view.restype = C.c_int
    view.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    dv, dd, mx = C.c_void_p(), C.c_void_p(), C.c_uint32()
    assert view(C.cast(ms, C.c_void_p), C.byref(dv), C.byref(dd), C.byref(mx)) == 0
    assert mx.value == oms.max
    v = np.empty(mx.value, np.uint64); d = np.empty(mx.value, np.uint16)
    mg.check(mg.lib().mgMemcpyD2H(v.ctypes.data, dv, v.nbytes, None)); mg.check(mg.lib().mgMemcpyD2H(d.ctypes.data, dd, d.nbytes, None))
    assert np.array_equal(v, oms.values()[1:]) and np.array_equal(d, oms.depths()[1:])


def read_sync0(ms, b, km, oms):
    mg.check(mg.lib().modsetSyncToHost(ms, 0))
    assert ms.contents.max == oms.max
    v, d, _ = mg.modset_arrays(ms)
    assert np.array_equal(v[1:], oms.values()[1:]) and np.array_equal(d[1:], oms.depths()[1:])


def read_sync1(ms, b, km, oms):
    assert_same_modset(ms, oms, BITS)


@pytest.mark.parametrize("va", MODES)
@pytest.mark.parametrize("reader", [read_find, read_query, read_hist, read_view, read_sync0, read_sync1], ids=lambda f: f.__name__)
def test_immediate_readers(va, reader, hashers, shared):
    """the call right after the add sees the finished values"""
    sh, _ = hashers
    b, km, oms = shared
    dr = DevReads(b)
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS)
        assert add_ok(ms, dr) == len(km)
        reader(ms, b, km, oms)
        assert_same_modset(ms, oms, BITS)
        mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("va", MODES)
def test_host_append(va, hashers):
    """entries appended on the host through the scalar API right after a device add are mirrored behind the add's values: both parts are there"""
    L = mg.lib()
    sh, oh = hashers
    b = synth_batch(700_000, 300_000, 79)
    extra = np.random.default_rng(7).integers(0, 1 << (2 * K), 500).astype(np.uint64)
    oms = oracle_build(oh, BITS, [b])
    want_extra = np.array([oms.find(int(x), True) for x in extra], np.uint32)
    assert (want_extra > 0).all()
    km = util.oracle_scan_batch(oh, *b)[0][:5000]
    want_km = np.array([oms.find(x) for x in km], np.uint32)
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS)
        add_ok(ms, DevReads(b))
        got_extra = np.array([L.modsetIndexFind(ms, int(x), 1) for x in extra], np.uint32)
        assert np.array_equal(got_extra, want_extra)
        assert np.array_equal(device_find(ms, np.concatenate([km, extra])), np.concatenate([want_km, want_extra]))
        assert_same_modset(ms, oms, BITS)
        L.modsetDestroy(ms)


@pytest.mark.parametrize("va", MODES)
def test_refused_add(va, hashers):
    """an add that does not fit the set's size is refused with MG_ERR_CAPACITY, the set answers as before the call, a smaller add then works"""
    L = mg.lib()
    sh, oh = hashers
    a, b, c = synth_batch(300_000, 100_000, 81), synth_batch(1_500_000, 500_000, 83), synth_batch(200_000, 80_000, 85)
    oa = oracle_build(oh, BITS, [a])
    size = oa.max + 20_000
    ka, kb = util.oracle_scan_batch(oh, *a)[0], util.oracle_scan_batch(oh, *b)[0][:20000]
    kb = np.setdiff1d(kb, ka)
    want_a = np.array([oa.find(x) for x in ka], np.uint32)
    oac = oracle_build(oh, BITS, [a, c])
    assert oracle_build(oh, BITS, [b]).max > size and oac.max < size
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS, size)
        add_ok(ms, DevReads(a))
        st, _ = DevReads(b).add(ms)
        assert st == MG_ERR_CAPACITY, (st, L.mgLastError())
        assert ms.contents.max == oa.max
        got = device_find(ms, np.concatenate([ka, kb]))
        assert np.array_equal(got[:len(ka)], want_a) and (got[len(ka):] == 0).all()
        add_ok(ms, DevReads(c))
        assert_same_modset(ms, oac, BITS)
        L.modsetDestroy(ms)


@pytest.mark.parametrize("va", MODES)
def test_destroy_and_rebuild(va, hashers, shared):
    """the set destroyed right after the add, another built in the same process: correct, and no error was set on the way (on a thread of
    its own: the library's last error is the calling thread's, and a new thread starts with none)"""
    sh, oh = hashers
    b, _, oms = shared
    b2 = synth_batch(400_000, 150_000, 87)
    oms2 = oracle_build(oh, BITS, [b2])
    failed = []

    def body():
        try:
            with knobs(va):
                ms = mg.modsetCreate(sh, BITS)
                add_ok(ms, DevReads(b))
                mg.lib().modsetDestroy(ms)
                ms = mg.modsetCreate(sh, BITS)
                add_ok(ms, DevReads(b2))
                assert_same_modset(ms, oms2, BITS)
                mg.lib().modsetDestroy(ms)
                assert mg.lib().mgLastError() == b""
        except BaseException as e:          # (handed to the test's own thread)
            failed.append(e)
    t = threading.Thread(target=body); t.start(); t.join()
    if failed:
        raise failed[0]


@pytest.mark.parametrize("va", MODES)
def test_caller_owned_kmers(va, hashers, shared):
    """modsetAddBatchDevice reads the caller's own array: overwritten right after the call returns, the values are those of before"""
    L = mg.lib()
    sh, oh = hashers
    km = shared[1][:70_001]
    oms = po.Modset(oh, BITS)
    for x in km:
        oms.find(int(x), True)
    d_k = mg.DeviceBuffer.from_numpy(km)
    junk = np.full(len(km), 0x155555555, np.uint64)
    with knobs(va):
        ms = mg.modsetCreate(sh, BITS)
        w0 = writers()
        mg.check(L.modsetAddBatchDevice(ms, d_k.ptr, len(km), None, 0, None))
        mg.check(L.mgMemcpyH2D(d_k.ptr, junk.ctypes.data, junk.nbytes, None))
        assert (writers() - w0).tolist() == ran(va)
        mg.check(L.modsetSyncToHost(ms, 0))
        assert ms.contents.max == oms.max
        assert np.array_equal(mg.modset_arrays(ms)[0][1:], oms.values()[1:])
        L.modsetDestroy(ms)


@pytest.mark.parametrize("va", MODES)
def test_segment_and_dense_sources(va, hashers, shared):
    """the writer reads the k-mers out of the scan's segments, or (MODGPU_NO_SEGMENT_INPUT=1) out of the dense array: the same set"""
    sh, _ = hashers
    b, _, oms = shared
    dr = DevReads(b)
    for dense in (None, 1):
        with knobs(va, NO_SEGMENT_INPUT=dense):
            ms = mg.modsetCreate(sh, BITS)
            add_ok(ms, dr)
            assert_same_modset(ms, oms, BITS)
            mg.lib().modsetDestroy(ms)


def test_which_path_ran(hashers, shared):
    """forced, disabled and left alone: the writer ran where the knob says.  Left alone it leaves the caller's stream for mgAddReadsDevice and
    stays on it for modsetAddBatchDevice, whose k-mers are the caller's; an add by the direct leg has no writer"""
    L = mg.lib()
    sh, _ = hashers
    b, km, _ = shared
    dr = DevReads(b)
    d_k = mg.DeviceBuffer.from_numpy(km[:50_000])
    for va, reads_ran, batch_ran in ((1, [1, 0], [1, 0]), (0, [0, 1], [0, 1]), (None, [1, 0], [0, 1])):
        with knobs(va):
            ms = mg.modsetCreate(sh, BITS)
            w0 = writers()
            add_ok(ms, dr)
            w1 = writers()
            mg.check(L.modsetAddBatchDevice(ms, d_k.ptr, 50_000, None, 0, None))
            w2 = writers()
            assert ((w1 - w0).tolist(), (w2 - w1).tolist()) == (reads_ran, batch_ran), va
            L.modsetDestroy(ms)
    with mg.knobs(VALUE_ASYNC=1, TABLE_PATH="direct"):
        ms = mg.modsetCreate(sh, BITS)
        w0 = writers()
        add_ok(ms, dr)
        assert (writers() - w0).tolist() == [0, 0]
        L.modsetDestroy(ms)
