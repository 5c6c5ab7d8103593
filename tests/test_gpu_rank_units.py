"""GPU: the ordered flag count (csrc/mg_rank.hip) with more than one row of 64 ordinals per rank unit.  The count is cut into at most
MG_RANK_UNITS = 8192 units, one per wave, so a unit has one row up to 8192 * 64 = 524 288 flags and the kernels' `row + j < rEnd` guards
decide nothing below that; every other test that reaches mgTablePrune does so with a few thousand entries.  Here a set of more than that
many entries is built by the direct leg (mgRankAssignKernel<true>), checked against the bucketed leg's build of the same batch
(mgRankRecordKernel + mgValueWriteKernel), and pruned by depth on the device (mgRankAssignKernel<false> + mgPruneMoveKernel): just over
8192 * 64 entries, two rows per unit, and just over nine times that, ten rows -- a second step of MG_RANK_ROWS = 8 rows with a partial tail."""
import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import synth

pytestmark = pytest.mark.gpu

K, D, SEED = 21, 4, 17
UNIT_ROW = 8192 * 64                  # MG_RANK_UNITS * 64: the flags of every unit's first row
READ = 10000
# rows per unit -> (bases of the iid genome, table bits).  One k-mer in D is a modimizer and nearly all of them are distinct, so the set
# ends a few per cent above (rows - 1) * UNIT_ROW entries
CASES = {2: (2_200_000, 22), 10: (19_600_000, 25)}


def batch(genome_bases):
    """the genome in reads of READ bases, then its first third once more: those k-mers end at depth 2, the others at 1"""
    g = synth.iid_bases(genome_bases, 23)
    bases = np.concatenate([g, g[:genome_bases // 3]])
    offs = np.unique(np.append(np.arange(0, len(bases), READ, dtype=np.int64), np.int64(len(bases))))
    return bases, offs


def build(path, bits, b):
    with mg.knobs(TABLE_PATH=path):
        ms = mg.modsetCreate(mg.seqhashCreate(K, D, SEED), bits)
        mg.add_sequence_batch(ms, *b)
        mg.check(mg.lib().modsetSyncToHost(ms, 0))
    return ms


def device_find(ms, kmers):
    d_p = mg.DeviceBuffer.from_numpy(kmers); d_o = mg.DeviceBuffer(len(kmers) * 4)
    mg.check(mg.lib().modsetFindBatchDevice(ms, d_p.ptr, len(kmers), d_o.ptr, None))
    return d_o.to_numpy(np.uint32, len(kmers))


@pytest.mark.parametrize("rows", sorted(CASES))
def test_build_and_prune_past_one_row_a_unit(rows):
    L = mg.lib()
    genome_bases, bits = CASES[rows]
    b = batch(genome_bases)
    other = build("bucket", bits, b)
    ov, od, _ = mg.modset_arrays(other)
    L.modsetDestroy(other)
    ms = build("direct", bits, b)
    v, d, info = mg.modset_arrays(ms)
    n = len(v) - 1
    print("rows per unit", rows, "entries", n)
    assert (rows - 1) * UNIT_ROW < n <= rows * UNIT_ROW, "the synthesis drifted: not %d rows per rank unit" % rows
    assert n % 64 != 0, "the synthesis drifted: the last row is full"
    # the two legs number the same first occurrences through different rank kernels
    assert len(ov) == len(v) and np.array_equal(v[1:], ov[1:]), "value[]: direct against bucketed"
    assert np.array_equal(d[1:], od[1:]), "depth[]: direct against bucketed"
    assert len(np.unique(v[1:])) == n and (d[1:] >= 1).all()

    keep = d[1:] >= 2
    m = int(keep.sum())
    print("survivors", m)
    assert 0 < m < n
    L.modsetDepthPrune(ms, 2, 0)
    mg.check(L.modsetSyncToHost(ms, 0))
    pv, pd, pi = mg.modset_arrays(ms)
    assert ms.contents.max == m and len(pv) == m + 1
    assert np.array_equal(pv[1:], v[1:][keep]), "value[] after the prune"
    assert np.array_equal(pd[1:], d[1:][keep]), "depth[] after the prune"
    assert np.array_equal(pi[1:], info[1:][keep]), "info[] after the prune"
    assert np.array_equal(device_find(ms, pv[1:]), np.arange(1, m + 1, dtype=np.uint32))
    L.modsetDestroy(ms)
