"""GPU: the device table on skewed keys, with proof of which kernel ran (mgTableDiag counts the launches).

The table hash is a fixed bijection, so k-mers can be written for any bucket (util.kmers_with_mix_prefix).  Three things the evenly
spread keys of the other suites cannot show:
  * the lookup paths: direct probes, one partition level, two levels over the 16-byte slots and over the 8-byte copy -- the last two
    need more than 512 buckets, which a small table has with 256 slots a bucket (MODGPU_BUCKET_R);
  * a change of geometry (a table regrown before lookups or by an add, a set the host built) sized by the MEAN bucket while one
    bucket holds far more than the mean;
  * the table after an add that was refused.
Every answer is compared with the oracle (oracle/pyoracle.py) or with the host's own arrays; the layout is checked by
mgTableCheckLayout, which does not use the lookups."""
import ctypes as C

import numpy as np
import pytest

import modimizer_amd as mg
from oracle import pyoracle as po
import util

pytestmark = pytest.mark.gpu

DIAG, diag = util.DIAG, util.table_diag
SMALL_R = dict(BUCKET_R=256, BUCKET_T=256)          # 256 slots a bucket: a table of a few hundred thousand slots has more than 512 buckets
DEFAULT_R = dict(BUCKET_R=None, BUCKET_T=None)      # (the geometries asserted are the defaults': tools/test_paths.sh runs the suite under sizing knobs)
MG_ERR_CAPACITY = 4


def layout(ms):
    out = (C.c_uint64 * 6)()
    mg.check(mg.lib().mgTableCheckLayout(ms, out))
    return [int(x) for x in out]


def device_add(ms, kmers, with_depth=0):
    d_k = mg.DeviceBuffer.from_numpy(kmers)
    return mg.lib().modsetAddBatchDevice(ms, d_k.ptr, len(kmers), None, with_depth, None)


def device_find(ms, kmers):
    d_p = mg.DeviceBuffer.from_numpy(kmers); d_o = mg.DeviceBuffer(len(kmers) * 4)
    mg.check(mg.lib().modsetFindBatchDevice(ms, d_p.ptr, len(kmers), d_o.ptr, None))
    return d_o.to_numpy(np.uint32, len(kmers))


class Reads:
    """a batch of reads on the device, for the scan-fed query"""
    def __init__(self, bases, offs):
        self.total, self.n = int(offs[-1]), len(offs) - 1
        self.d_p = mg.DeviceBuffer.from_numpy(mg.pack_host(bases)); self.d_o = mg.DeviceBuffer.from_numpy(offs.astype(np.uint64))


def query_reads(ms, reads, n_seeds):
    """mgQueryReadsDevice: the index of every modimizer of the reads, in order"""
    cap = n_seeds + 8
    d_ix = mg.DeviceBuffer(cap * 4)
    n = C.c_uint64()
    mg.check(mg.lib().mgQueryReadsDevice(ms, reads.d_p.ptr, reads.total, reads.d_o.ptr, reads.n, d_ix.ptr, None, None, cap, C.byref(n), None))
    assert n.value == n_seeds, "the scan found other modimizers than the oracle"
    return d_ix.to_numpy(np.uint32, n_seeds)


def oracle_set(oh, bits, kmers, size=0):
    oms = po.Modset(oh, bits, size)
    for x in kmers:
        oms.find(int(x), True)
    return oms


def oracle_answers(oms, q):
    """modsetIndexFind (oms, x, false) for every x of q, from the oracle's own value[]"""
    v = oms.values()[1:]
    order = np.argsort(v, kind="stable"); vs = v[order]
    at = np.minimum(np.searchsorted(vs, q), len(vs) - 1)
    return np.where(vs[at] == q, order[at] + 1, 0).astype(np.uint32)


def assert_same_modset(ms, oms, bits, depth=None):
    """depth: what every entry's depth must be where the device add counted (the oracle's find (x, true) creates entries at depth 0)"""
    mg.check(mg.lib().modsetSyncToHost(ms, 1))
    assert ms.contents.max == oms.max
    v, d, _ = mg.modset_arrays(ms)
    assert np.array_equal(v[1:], oms.values()[1:]), "values"
    want_d = oms.depths()[1:] if depth is None else np.full(oms.max, depth, np.uint16)
    assert np.array_equal(d[1:], want_d), "depths: %d entries differ" % int((d[1:] != want_d).sum())
    assert np.array_equal(np.ctypeslib.as_array(ms.contents.index, (1 << bits,)), oms.index_table()), "index[]"


def spread_kmers(rng, n, k, avoid=None):
    """n distinct random k-mers; avoid = (prefix, bits): none of them in that bucket of a table of 2^bits buckets"""
    x = np.unique(rng.integers(0, 1 << (2 * k), n * 2 + 64, dtype=np.uint64))
    if avoid is not None:
        x = x[util.bucket_of(x, k, avoid[1]) != avoid[0]]
    x = rng.permutation(x)[:n]
    assert len(x) == n
    return x


def canonical(oh, cand, k, at_least):
    kept, bases, offs = util.kmer_reads(oh, cand, k)
    assert len(kept) >= at_least, "the crafted set is smaller than it should be: %d of %d candidates came out of the scan unchanged" % (len(kept), len(cand))
    return kept


FIND_PATHS = [("direct", 1, "direct"), ("part", 1, "part1"), ("2", 0, "part2_16"), ("2", 1, "part2_8")]


def expect_counter(path_counter, rem_bits):
    """two levels read the 8-byte copy only where the key's bits below the bucket id fit 32"""
    return "part2_16" if path_counter == "part2_8" and rem_bits > 32 else path_counter


def ask_every_path(ms, reads, n_seeds, want, rem_bits, what):
    """the same reads through the four lookup paths: each must run the kernel it is named after and give the oracle's answers"""
    answers = {}
    for path, find8, counter in FIND_PATHS:
        counter = expect_counter(counter, rem_bits)
        with mg.knobs(FIND_PATH=path, FIND8=find8):
            before = diag(ms)
            got = query_reads(ms, reads, n_seeds)
            after = diag(ms)
        print(what, "FIND_PATH", path, "FIND8", find8, "launches", {c: after[c] - before[c] for c in DIAG[2:]}, "wrong answers", int((got != want).sum()))
        ran = {c for c in DIAG[2:6] if after[c] != before[c]}
        assert ran == {counter}, "%s: FIND_PATH=%s FIND8=%d ran %s, not %s (geometry 2^%d x %d)" % (what, path, find8, sorted(ran), counter, after["log2NB"], after["R"])
        answers[(path, find8)] = got
    for key, got in answers.items():
        assert np.array_equal(got, want), "%s: %s disagrees with the oracle in %d of %d answers" % (what, key, int((got != want).sum()), len(want))
    return answers


# ---------------------------------------------------------------------------------------------------------------------------------
# lookup paths really taken

# (k, entries): 2k - log2 NB = 31, 32, 33 and well above (43) in the geometry util.table_geometry says (asserted against the table's own)
LOOKUP_CASES = [(21, 200_000, 11, 31), (21, 100_000, 10, 32), (22, 200_000, 11, 33), (27, 200_000, 11, 43)]


@pytest.mark.parametrize("k,entries,log2nb,rem", LOOKUP_CASES)
def test_lookup_paths_really_taken(k, entries, log2nb, rem):
    """a table of more than 512 buckets at small size; present and absent k-mers through the scan-fed query under every lookup path;
    the 8-byte copy is made once, reused by the next batch and made again after an add; a pipelined pair on the two-level path"""
    L = mg.lib()
    bits = 22
    rng = np.random.default_rng(k * 7 + log2nb)
    sh = mg.seqhashCreate(k, 1, 17); oh = po.Hasher(k, 1, 17)
    assert util.table_geometry(util.slots_for(entries, util.LOOKUP_LOAD, bits), 256) == (log2nb, 256)
    pool = spread_kmers(rng, entries + 60_000, k)
    members, others = pool[:entries], pool[entries:]
    present = canonical(oh, members[:40_000], k, 15_000)[:14_000]
    absent = canonical(oh, others[:40_000], k, 15_000)
    late = absent[14_000:15_000]                          # added later: absent for the first batches, present afterwards
    absent = absent[:14_000]
    q = rng.permutation(np.concatenate([present, absent, late]))
    _, qb, qo = util.kmer_reads(oh, q, k)
    assert len(qo) - 1 == len(q)
    with mg.knobs(TABLE_LOAD=util.LOOKUP_LOAD, TIGHT_LOAD=0, **SMALL_R):
        ms = mg.modsetCreate(sh, bits)
        assert device_add(ms, members) == 0
        oms = oracle_set(oh, bits, members)
        d0 = diag(ms)
        assert (d0["log2NB"], d0["R"]) == (log2nb, 256) and 2 * k - d0["log2NB"] == rem, d0
        reads = Reads(qb, qo)
        want = oracle_answers(oms, q)
        assert (want != 0).sum() == len(present) and (want == 0).sum() == len(absent) + len(late)
        ask_every_path(ms, reads, len(q), want, rem, "k=%d" % k)
        if (k, entries, rem) == (21, 200_000, 31):
            # the scatter and the pulls at the small sub-chunk size (by default only the 16384-element instances run), and the second
            # pass counting its digits from the elements instead of the bytes the first pass leaves
            for knob in ({"PART_BIG": 0}, {"PART_DIGITS": 0}):
                with mg.knobs(**knob):
                    ask_every_path(ms, reads, len(q), want, rem, "k=%d %s" % (k, knob))
            # a batch that ends exactly on a tile boundary of the pulls (16384 results a tile), and one result beyond it
            for m in (16384, 16384 + 1):
                _, sb, so = util.kmer_reads(oh, q[:m], k)
                assert len(so) - 1 == m
                ask_every_path(ms, Reads(sb, so), m, want[:m], rem, "k=%d, %d lookups" % (k, m))
        assert layout(ms)[:4] == [0, 0, 0, oms.max]
        with mg.knobs(FIND_PATH="2", FIND8=1):
            d1 = diag(ms)
            assert d1["pack8"] == (1 if rem <= 32 else 0), d1
            # a second batch on the same table reuses the copy
            q2 = q[::-1].copy()
            _, q2b, q2o = util.kmer_reads(oh, q2, k)
            assert np.array_equal(query_reads(ms, Reads(q2b, q2o), len(q2)), want[::-1])
            assert diag(ms)["pack8"] == d1["pack8"], "the 8-byte copy was made again for a table that had not changed"
            # an add changes the table: the next batch must see the new entries
            assert device_add(ms, late) == 0
            for x in late:
                oms.find(int(x), True)
            want = oracle_answers(oms, q)
            assert (want != 0).sum() == len(present) + len(late)
            # ... through a pipelined pair: both scans started before the first lookups run
            outs = [mg.DeviceBuffer((len(q) + 8) * 4) for _ in range(2)]
            tickets = [C.c_void_p(), C.c_void_p()]
            r2 = Reads(q2b, q2o)
            before = diag(ms)
            mg.check(L.mgQueryReadsDeviceAsync(ms, reads.d_p.ptr, reads.total, reads.d_o.ptr, reads.n, outs[0].ptr, None, None, len(q) + 8, C.byref(tickets[0]), None))
            mg.check(L.mgQueryReadsDeviceAsync(ms, r2.d_p.ptr, r2.total, r2.d_o.ptr, r2.n, outs[1].ptr, None, None, len(q) + 8, C.byref(tickets[1]), None))
            n = C.c_uint64()
            mg.check(L.mgQueryReadsDeviceWait(tickets[0], C.byref(n), None)); assert n.value == len(q)
            mg.check(L.mgQueryReadsDeviceWait(tickets[1], C.byref(n), None)); assert n.value == len(q)
            after = diag(ms)
            two = "part2_8" if rem <= 32 else "part2_16"
            assert after[two] - before[two] == 2 and after["pack8"] - before["pack8"] == (1 if rem <= 32 else 0), (before, after)
            assert np.array_equal(outs[0].to_numpy(np.uint32, len(q)), want), "first of the pair"
            assert np.array_equal(outs[1].to_numpy(np.uint32, len(q)), want[::-1]), "second of the pair"
        assert layout(ms)[:4] == [0, 0, 0, oms.max]
        assert_same_modset(ms, oms, bits)
        L.modsetDestroy(ms)


# ---------------------------------------------------------------------------------------------------------------------------------
# near-full buckets on every path

@pytest.mark.parametrize("table_path", ["bucket", "direct"])
def test_near_full_bucket_on_every_path(table_path):
    """one bucket of a 1024 x 256 table holds R - 1 keys -- every probe chain in it is long and wraps at the bucket's end -- beside
    evenly filled ones.  Every lookup path is asked for each of them and for as many absent k-mers of the same bucket: the answers,
    not only the return, are checked.  One more key fills the bucket (a later add claims slots one by one, and takes R keys: on the
    card the refusal at R keys is the scan placement's alone); an absent k-mer then walks all R slots and must still come back with
    0.  The key after that is refused: the bucket did hold R."""
    L = mg.lib()
    k, bits, R, hot_bucket = 21, 22, 256, 0x2a5
    rng = np.random.default_rng(77)
    sh = mg.seqhashCreate(k, 1, 17); oh = po.Hasher(k, 1, 17)
    entries = 100_000
    assert util.table_geometry(util.slots_for(entries, util.LOOKUP_LOAD, bits), 256) == (10, R)
    hot_pool = canonical(oh, util.kmers_with_mix_prefix(rng, 1400, hot_bucket, 10, k), k, 2 * R)
    hot_in, hot_out, one_more, too_many = hot_pool[:R - 1], hot_pool[R - 1:2 * R - 2], hot_pool[2 * R - 2:2 * R - 1], hot_pool[2 * R - 1:2 * R]
    pool = spread_kmers(rng, entries + 30_000, k, avoid=(hot_bucket, 10))
    even, others = pool[:entries - (R - 1)], pool[entries:]
    members = rng.permutation(np.concatenate([even, hot_in]))
    present = canonical(oh, even[:12_000], k, 4000)[:4000]
    absent = canonical(oh, others[:12_000], k, 4000)[:4000]
    q = rng.permutation(np.concatenate([hot_in, hot_out, present, absent, one_more, too_many]))
    _, qb, qo = util.kmer_reads(oh, q, k)
    with mg.knobs(TABLE_LOAD=util.LOOKUP_LOAD, TIGHT_LOAD=0, TABLE_PATH=table_path, MERGE_SLOTS=0, **SMALL_R):
        ms = mg.modsetCreate(sh, bits)
        assert device_add(ms, members) == 0, L.mgLastError()
        oms = oracle_set(oh, bits, members)
        d0 = diag(ms)
        assert (d0["log2NB"], d0["R"]) == (10, R), d0
        lay = layout(ms)
        assert lay[:4] == [0, 0, 0, entries], lay
        want = oracle_answers(oms, q)
        is_hot_in = np.isin(q, hot_in); is_hot_out = np.isin(q, hot_out)
        assert (want[is_hot_in] != 0).all() and (want[is_hot_out] == 0).all() and is_hot_in.sum() == R - 1 and is_hot_out.sum() == R - 1
        assert (want[np.isin(q, np.concatenate([one_more, too_many]))] == 0).all()
        ask_every_path(ms, Reads(qb, qo), len(q), want, 2 * k - 10, "near-full, built by " + table_path)
        assert np.array_equal(device_find(ms, q), want)
        assert layout(ms)[:4] == [0, 0, 0, entries]
        # the bucket full to its last slot
        assert device_add(ms, one_more) == 0, L.mgLastError()
        oms.find(int(one_more[0]), True)
        assert layout(ms)[:4] == [0, 0, 0, entries + 1]
        want = oracle_answers(oms, q)
        assert want[q == one_more[0]][0] == entries + 1 and (want[is_hot_out] == 0).all()
        ask_every_path(ms, Reads(qb, qo), len(q), want, 2 * k - 10, "full bucket, built by " + table_path)
        assert np.array_equal(device_find(ms, q), want)
        st = device_add(ms, too_many)
        assert st == MG_ERR_CAPACITY, "a bucket of R keys took one more (status %d): it did not hold R" % st
        assert layout(ms)[:4] == [0, 0, 0, entries + 1]
        ask_every_path(ms, Reads(qb, qo), len(q), want, 2 * k - 10, "full bucket after a refused key, built by " + table_path)
        assert_same_modset(ms, oms, bits)
        L.modsetDestroy(ms)


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry changes under skew

def check_complete(ms, oms, bits, what, depth=None):
    """after a change of geometry: every entry found on the device under its own index, the set equal to the oracle's (depth: see
    assert_same_modset), and a second add of all its k-mers, without counting, creates nothing"""
    L = mg.lib()
    lay = layout(ms)
    v = oms.values()[1:].copy()
    got = device_find(ms, v)
    lost = int((got != np.arange(1, len(v) + 1)).sum())
    print(what, "geometry", diag(ms), "layout", lay, "entries", oms.max, "not found under their index", lost)
    assert lost == 0, "%s: %d of %d entries are not found on the device" % (what, lost, len(v))
    assert lay[:4] == [0, 0, 0, oms.max], (what, lay)
    assert_same_modset(ms, oms, bits, depth)
    assert device_add(ms, v) == 0, L.mgLastError()
    assert ms.contents.max == oms.max, "%s: adding the set's own k-mers again created %d entries" % (what, ms.contents.max - oms.max)
    assert_same_modset(ms, oms, bits, depth)


def rehash_counter(table_path):
    return "rehash_bucket" if table_path == "bucket" else "rehash_atomic"


def skewed(rng, k, n, hot, prefix, prefix_bits, parent_bits, even=False):
    """n k-mers: `hot` of them under one prefix, the others anywhere but in that prefix's bucket of the table of 2^parent_bits buckets
    the set is built in (which so holds the hot ones alone); even: the control, all of them spread evenly"""
    if even:
        return spread_kmers(rng, n, k)
    hot_k = util.kmers_with_mix_prefix(rng, hot, prefix, prefix_bits, k)
    rest = spread_kmers(rng, n - hot, k, avoid=(prefix >> (prefix_bits - parent_bits), parent_bits))
    return rng.permutation(np.concatenate([hot_k, rest]))


GROWTH = [
    # name, knobs, entries, hot keys, their prefix bits, buckets before (log2), geometry before, after
    ("default R", DEFAULT_R, 30_000, 2500, 5, 4, (4, 4096), (5, 2368)),
    ("R = 256", SMALL_R, 39_000, 200, 9, 8, (8, 256), (9, 192)),
]


@pytest.mark.parametrize("even", [False, True], ids=["skewed", "control"])
@pytest.mark.parametrize("table_path", ["bucket", "direct"])
@pytest.mark.parametrize("case", GROWTH, ids=[c[0] for c in GROWTH])
def test_lookup_triggered_growth(case, table_path, even):
    """a set built at load 0.6 is brought to load 0.4 by its first lookup batch: more buckets of fewer slots, sized by the mean.  One
    bucket of the old table holds more keys under one longer prefix than a new bucket has slots.  Nothing may be lost.  The control
    has the same counts spread evenly."""
    name, knobs, entries, hot, pb, parent_bits, geom0, geom1 = case
    k, bits = 21, 22
    rng = np.random.default_rng(entries + hot)
    sh = mg.seqhashCreate(k, 4, 17); oh = po.Hasher(k, 4, 17)
    members = skewed(rng, k, entries, hot, 1, pb, parent_bits, even)
    with mg.knobs(TABLE_LOAD=None, TIGHT_LOAD=0, TABLE_PATH="bucket", **knobs):
        ms = mg.modsetCreate(sh, bits)
        assert device_add(ms, members, 1) == 0
        oms = oracle_set(oh, bits, members)
        d0 = diag(ms)
        assert (d0["log2NB"], d0["R"]) == geom0, d0
        assert layout(ms)[:4] == [0, 0, 0, entries]
        with mg.knobs(TABLE_PATH=table_path):
            probe = device_find(ms, members[:64])
        d1 = diag(ms)
        print(name, table_path, "even" if even else "skewed", "before", d0, "after", d1)
        c = rehash_counter(table_path)
        assert d1[c] - d0[c] >= 1 and (d1["rehash_bucket"] + d1["rehash_atomic"]) > (d0["rehash_bucket"] + d0["rehash_atomic"]), "the lookup did not change the geometry with the %s kernel" % c
        if even:
            assert (d1["log2NB"], d1["R"]) == geom1, d1
        assert d1["R"] << d1["log2NB"] >= entries * 100 // util.LOOKUP_LOAD
        assert np.array_equal(probe, oracle_answers(oms, members[:64]))
        check_complete(ms, oms, bits, "%s, %s, %s" % (name, table_path, "even" if even else "skewed"), depth=1)      # (the add counted every k-mer once: the counts move with the entries)
        mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("even", [False, True], ids=["skewed", "control"])
@pytest.mark.parametrize("chunk", [None, 20_000], ids=["one chunk", "chunked"])
@pytest.mark.parametrize("table_path", ["bucket", "direct"])
def test_add_triggered_growth_beyond_doubling(table_path, chunk, even):
    """30 000 entries in 16 x 4096 slots take 60 000 more: 64 x 2368 in one step (more than doubled, so R shrinks) -- or, added in
    chunks, by doubling between the chunks.  2500 of the first entries share a 6-bit prefix."""
    k, bits = 21, 22
    rng = np.random.default_rng(606)
    sh = mg.seqhashCreate(k, 4, 17); oh = po.Hasher(k, 4, 17)
    first = skewed(rng, k, 30_000, 2500, 9, 6, 4, even)
    more = spread_kmers(rng, 70_000, k, avoid=None if even else (9, 6))
    more = more[~np.isin(more, first)][:60_000]
    assert len(more) == 60_000
    with mg.knobs(TABLE_LOAD=None, TIGHT_LOAD=0, TABLE_PATH="bucket", **DEFAULT_R):
        ms = mg.modsetCreate(sh, bits)
        assert device_add(ms, first) == 0
        d0 = diag(ms)
        assert (d0["log2NB"], d0["R"]) == (4, 4096), d0
        with mg.knobs(TABLE_PATH=table_path, ADD_CHUNK=chunk):
            st = device_add(ms, more)
        assert st == 0, mg.lib().mgLastError()
        d1 = diag(ms)
        print(table_path, chunk, "even" if even else "skewed", "before", d0, "after", d1)
        c = rehash_counter(table_path)
        assert d1[c] - d0[c] >= (2 if chunk else 1), "the add did not change the geometry with the %s kernel: %s" % (c, d1)
        if even and not chunk:
            assert (d1["log2NB"], d1["R"]) == (6, 2368), d1
        oms = oracle_set(oh, bits, np.concatenate([first, more]))
        with mg.knobs(TABLE_PATH="bucket"):
            check_complete(ms, oms, bits, "add-triggered, %s, chunk %s, %s" % (table_path, chunk, "even" if even else "skewed"))
        mg.lib().modsetDestroy(ms)


@pytest.mark.parametrize("even", [False, True], ids=["skewed", "control"])
@pytest.mark.parametrize("how", ["scalar", "file"])
def test_host_built_set_first_meets_a_lookup(how, even, tmp_path):
    """a set the host filled (modsetIndexFind (.., true) calls, or a .mod file read back) is mirrored on the device at its first
    batch call, into a table sized by its entry count: 16 x 4096 for 30 000.  4300 of them share a 4-bit prefix."""
    L = mg.lib()
    k, bits = 21, 22
    rng = np.random.default_rng(4300)
    sh = mg.seqhashCreate(k, 4, 17); oh = po.Hasher(k, 4, 17)
    members = skewed(rng, k, 30_000, 4300, 6, 4, 4, even)
    with mg.knobs(TABLE_LOAD=None, TIGHT_LOAD=0, TABLE_PATH=None, **DEFAULT_R):
        ms = mg.modsetCreate(sh, bits)
        for x in members:
            assert L.modsetIndexFind(ms, int(x), 1)
        if how == "file":
            path = str(tmp_path / "skew.mod")
            with mg.CFile(path, "w") as f:
                L.modsetWrite(ms, f)
            L.modsetDestroy(ms)
            with mg.CFile(path, "r") as f:
                ms = L.modsetRead(f)
            assert ms and ms.contents.max == len(members)
        assert diag(ms)["R"] == 0, "the set has a device table before its first batch call"
        oms = oracle_set(oh, bits, members)
        got = device_find(ms, members)                       # the first device call is a lookup batch
        lost = int((got != np.arange(1, len(members) + 1)).sum())
        print(how, "even" if even else "skewed", diag(ms), "not found", lost)
        assert lost == 0, "%d of %d entries of the host's set are not found on the device" % (lost, len(members))
        check_complete(ms, oms, bits, "host-built (%s), %s" % (how, "even" if even else "skewed"))
        L.modsetDestroy(ms)


@pytest.mark.parametrize("even", [False, True], ids=["skewed", "control"])
def test_host_adds_between_device_calls(even):
    """entries added through the scalar API while the set has a device table are mirrored at the next batch call, into the table as
    it is: 20 000 entries in 16 x 4096 slots take 3000 more that share a 4-bit prefix (the control: 3000 spread evenly)"""
    L = mg.lib()
    k, bits = 21, 22
    rng = np.random.default_rng(3000)
    sh = mg.seqhashCreate(k, 4, 17); oh = po.Hasher(k, 4, 17)
    first = spread_kmers(rng, 20_000, k)
    late = util.kmers_with_mix_prefix(rng, 3100, 11, 4, k) if not even else spread_kmers(rng, 3100, k)
    late = late[~np.isin(late, first)][:3000]
    with mg.knobs(TABLE_LOAD=None, TIGHT_LOAD=0, TABLE_PATH=None, **DEFAULT_R):
        ms = mg.modsetCreate(sh, bits)
        assert device_add(ms, first) == 0
        assert np.array_equal(device_find(ms, first[:100]), np.arange(1, 101))
        d0 = diag(ms)
        assert (d0["log2NB"], d0["R"]) == (4, 4096), d0
        for i, x in enumerate(late):
            assert L.modsetIndexFind(ms, int(x), 1) == 20_001 + i
        oms = oracle_set(oh, bits, np.concatenate([first, late]))
        got = device_find(ms, late)
        lost = int((got != np.arange(20_001, 23_001)).sum())
        print("even" if even else "skewed", "before", d0, "after", diag(ms), "not found", lost)
        assert lost == 0, "%d of %d entries the host added are not found on the device" % (lost, len(late))
        check_complete(ms, oms, bits, "host adds between device calls, %s" % ("even" if even else "skewed"))
        L.modsetDestroy(ms)


@pytest.mark.parametrize("how", ["rehash", "host-built"])
def test_no_legal_geometry_leaves_the_set_answering(how):
    """MG_ERR_CAPACITY where no legal geometry holds the entries (a bucket has at most 8192 slots, a table of 22 bits at most 2^21: 256
    buckets of that size, and k-mers that share ten bits of their hash share a bucket in every one of them).
    rehash: 8 buckets of 8192 slots, one filled to its last slot by the atomic insert; the first lookup batch wants load 0.4, no
    geometry keeps a slot free beside 8192 keys, the call fails -- and the old table is still there: at a load that asks for no
    growth every entry is found, and the layout is as before.
    host-built: 8300 such k-mers among 28 000 scalar adds; the first batch call cannot mirror the set and says so, the set has no
    device table, and the host goes on answering."""
    L = mg.lib()
    k, bits = 21, 22
    rng = np.random.default_rng(8192)
    sh = mg.seqhashCreate(k, 4, 17)
    hot = util.kmers_with_mix_prefix(rng, 8192 if how == "rehash" else 8300, 0x3ff, 10, k)
    members = rng.permutation(np.concatenate([hot, spread_kmers(rng, 20_000, k, avoid=(7, 3))]))
    if how == "rehash":
        with mg.knobs(TABLE_LOAD=None, TIGHT_LOAD=0, TABLE_PATH="direct", BUCKET_R=8192, BUCKET_T=None):
            ms = mg.modsetCreate(sh, bits)
            assert device_add(ms, members) == 0, L.mgLastError()
            d0, lay0 = diag(ms), layout(ms)
            assert (d0["log2NB"], d0["R"]) == (3, 8192) and lay0[:4] == [0, 0, 0, len(members)], (d0, lay0)
            d_p = mg.DeviceBuffer.from_numpy(members); d_o = mg.DeviceBuffer(len(members) * 4)
            st = L.modsetFindBatchDevice(ms, d_p.ptr, len(members), d_o.ptr, None)
            assert st == MG_ERR_CAPACITY and b"no geometry" in L.mgLastError(), (st, L.mgLastError())
            with mg.knobs(TABLE_LOAD=100):
                d1 = diag(ms)
                assert (d1["log2NB"], d1["R"]) == (3, 8192) and d1["rehash_bucket"] + d1["rehash_atomic"] > d0["rehash_bucket"] + d0["rehash_atomic"], d1
                assert layout(ms) == lay0
                assert np.array_equal(device_find(ms, members), np.arange(1, len(members) + 1))
                absent = np.concatenate([spread_kmers(rng, 3000, k), util.kmers_with_mix_prefix(rng, 300, 0x3ff, 10, k)])      # (those walk all 8192 slots of the full bucket)
                absent = absent[~np.isin(absent, members)]
                assert len(absent) > 3200 and (device_find(ms, absent) == 0).all()
                assert ms.contents.max == len(members)
    else:
        with mg.knobs(TABLE_LOAD=None, TIGHT_LOAD=0, TABLE_PATH=None, **DEFAULT_R):
            ms = mg.modsetCreate(sh, bits)
            for x in members:
                assert L.modsetIndexFind(ms, int(x), 1)
            d_p = mg.DeviceBuffer.from_numpy(members); d_o = mg.DeviceBuffer(len(members) * 4)
            st = L.modsetFindBatchDevice(ms, d_p.ptr, len(members), d_o.ptr, None)
            assert st == MG_ERR_CAPACITY and b"no geometry" in L.mgLastError(), (st, L.mgLastError())
            assert diag(ms)["R"] == 0 and L.mgModsetDeviceSlots(ms) == 0, "a device table that does not hold the set was kept"
            assert ms.contents.max == len(members)
            assert all(L.modsetIndexFind(ms, int(x), 0) == i + 1 for i, x in enumerate(members[:2000]))
    L.modsetDestroy(ms)


# ---------------------------------------------------------------------------------------------------------------------------------
# after a refused add

@pytest.mark.parametrize("kind", ["size", "R + 1 keys, MERGE_PLACE=0", "R keys, MERGE_PLACE=1"])
def test_after_a_refused_add(kind):
    """an add that fails with MG_ERR_CAPACITY -- the set's size would be reached, or one bucket is offered more keys than it takes:
    as many as it has slots where the merge kernel lays a fresh bucket out by prefix scan (MERGE_PLACE=1), one more where it claims
    slots one by one (MERGE_PLACE=0: R keys are taken, seen on the card, and fill the bucket to its last slot) -- leaves a set a
    caller that handles the error goes on using: max and the host arrays as before, every earlier entry
    answered with its index and every k-mer of the refused batch that was not in the set with 0, by every lookup path alike.
    (The refused batch is added without depth counting: what it counted before the refusal is not part of this contract.)"""
    L = mg.lib()
    k, bits, R, hot_bucket = 21, 22, 256, 0x133
    rng = np.random.default_rng(len(kind))
    sh = mg.seqhashCreate(k, 1, 17); oh = po.Hasher(k, 1, 17)
    entries = 100_000
    size = entries + 600 if kind == "size" else 0
    pool = spread_kmers(rng, entries + 30_000, k, avoid=(hot_bucket, 10))
    members, others = pool[:entries], pool[entries:]
    present = canonical(oh, members[:12_000], k, 4000)[:4000]
    if kind == "size":
        refused = canonical(oh, others[:6000], k, 2000)[:2000]                 # 2000 new k-mers where 599 have room
        refused = np.concatenate([refused, present[:300]])                      # and some the set has already
    else:
        refused = canonical(oh, util.kmers_with_mix_prefix(rng, 800, hot_bucket, 10, k), k, R + 1)[:R + 1 if kind.startswith("R + 1") else R]
    absent = canonical(oh, others[6000:18_000], k, 4000)[:4000]
    q = rng.permutation(np.unique(np.concatenate([present, absent, refused])))
    _, qb, qo = util.kmer_reads(oh, q, k)
    place = 1 if kind.endswith("=1") else 0
    with mg.knobs(TABLE_LOAD=util.LOOKUP_LOAD, TIGHT_LOAD=0, TABLE_PATH="bucket", MERGE_SLOTS=0, MERGE_PLACE=place, **SMALL_R):
        ms = mg.modsetCreate(sh, bits, size)
        assert device_add(ms, members) == 0, L.mgLastError()
        oms = oracle_set(oh, bits, members)
        assert_same_modset(ms, oms, bits)
        d0 = diag(ms)
        assert (d0["log2NB"], d0["R"]) == (10, R), d0
        st = device_add(ms, refused)
        assert st == MG_ERR_CAPACITY, (st, L.mgLastError())
        assert ms.contents.max == entries
        assert_same_modset(ms, oms, bits)
        lay = layout(ms)
        print(kind, "layout after the refusal", lay, diag(ms))
        assert lay[:4] == [0, 0, 0, entries], "what the refused add wrote is still in the table: %s" % lay
        want = oracle_answers(oms, q)
        assert (want[np.isin(q, refused) & ~np.isin(q, present)] == 0).all()
        direct = device_find(ms, q)
        print(kind, "modsetFindBatchDevice: wrong answers", int((direct != want).sum()), "of them for k-mers of the refused batch", int((direct != want)[np.isin(q, refused)].sum()))
        answers = ask_every_path(ms, Reads(qb, qo), len(q), want, 2 * k - 10, "after a refused add (%s)" % kind)
        assert np.array_equal(direct, want)
        assert all(np.array_equal(a, direct) for a in answers.values())
        # the set goes on: what fits is taken
        fits = refused[:200] if kind == "size" else refused[:-1]
        assert device_add(ms, fits) == 0, L.mgLastError()
        for x in fits:
            oms.find(int(x), True)
        assert layout(ms)[:4] == [0, 0, 0, oms.max]
        want = oracle_answers(oms, q)
        ask_every_path(ms, Reads(qb, qo), len(q), want, 2 * k - 10, "after the add that fits (%s)" % kind)
        assert_same_modset(ms, oms, bits)
        L.modsetDestroy(ms)
