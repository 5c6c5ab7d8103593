"""GPU: the filter mode's two threshold tests -- four starts' top bytes packed into one register (d <= 256, csrc/mg_packedtest.h) and
every start compared on its own -- give the oracle's stream, bit for bit, wherever the filter runs.

The pairs: k from 17 to 32 and d = 2^m, m from 3 to 12, of which the filter (MG_MODE_FAST, csrc/mg_scan.hip) takes those with
64 - 2k + m <= 32.  PAIRS is written from that threshold; test_the_pairs_are_where_fast_runs scans with every pair of the range and
holds PAIRS against what mgScanDiag says ran, so no case below can meet another mode -- each asserts FAST all the same.  (k = 32 is
in the range and in no pair: seqhashCreate takes k < 32, as the reference's does.)  m <= 8 tests the top byte and has the packed
test, m >= 9 never has it; MODGPU_SCAN_PACKED_TEST=0 takes it away everywhere.  mgScanTailDiag proves which of the two ran.

Every pair, with the knob at 1 and at 0, runs seven batches of about 13 000 bases through both instances of the kernel: the one with
positions and read ids (seqhashScanBatch: k-mer, pos, strand, read against the oracle's) and the one for the k-mers alone
(mgAddReadsDevice into a set of 2^20 slots, the set's k-mers and depths against the oracle's set).  One worker owns the batch's four
tiles (MODGPU_SCAN_GRID=1), so the candidates a tile leaves waiting cross into the next."""
import ctypes as C
import functools

import numpy as np
import pytest

import modimizer_amd as mg
from oracle import pyoracle as po
import util

pytestmark = pytest.mark.gpu
SEED, BITS = 17, 20
KS, MS = range(17, 33), range(3, 13)
PAIRS = [(k, m) for k in KS for m in MS if k < 32 and 64 - 2 * k + m <= 32]
LENS = [5000, 70, 20, 8000]          # 20 < k from k = 21 up; the reads' ends at 5000, 5070 and 5090 fall into two lanes' 64 starts


def test_the_pairs_cover_both_tails():
    ms = {m for _, m in PAIRS}
    assert {3, 8, 9} <= ms and len(PAIRS) == 120
    assert (18, 3) in PAIRS and (17, 3) not in PAIRS and (20, 8) in PAIRS and (20, 9) not in PAIRS and (21, 9) in PAIRS


@functools.lru_cache(maxsize=1)
def batches():
    """the seven batches: made once, only read"""
    out = []
    for seed in range(1, 6):
        rng = np.random.default_rng(seed)
        out.append(("random%d" % seed, util.concat_reads([rng.integers(0, 4, n).astype(np.uint8) for n in LENS])))
    out.append(("polyA", util.concat_reads([np.zeros(9000, np.uint8)])))          # every product 0: every start a candidate, listed in passes
    r = np.random.default_rng(6).integers(0, 4, 6500).astype(np.uint8)
    out.append(("revcomp", util.concat_reads([r, (3 - r[::-1]).astype(np.uint8)])))    # both strands of every k-mer pass together
    return out


class DevReads:
    """a batch packed and on the device, as mgAddReadsDevice takes it"""

    def __init__(self, bases, offs):
        self.total, self.n_reads = int(offs[-1]), len(offs) - 1
        self.d_p = mg.DeviceBuffer.from_numpy(mg.pack_host(bases))
        self.d_o = mg.DeviceBuffer.from_numpy(offs.astype(np.uint64))

    def add(self, ms):
        n = C.c_uint64()
        mg.check(mg.lib().mgAddReadsDevice(ms, self.d_p.ptr, self.total, self.d_o.ptr, self.n_reads, C.byref(n), None))
        return n.value


@functools.lru_cache(maxsize=1)
def dev_batches():
    return [DevReads(*b) for _, b in batches()]


def tails():
    """mgScanTailDiag: FAST launches (with the packed test, with the test per start) since the process started"""
    out = (C.c_uint64 * 2)()
    mg.check(mg.lib().mgScanTailDiag(out))
    return [int(out[0]), int(out[1])]


def tails_since(before):
    return [a - b for a, b in zip(tails(), before)]


def set_pairs(values, depths):
    """a set's (k-mer, depth) pairs in k-mer order"""
    o = np.argsort(values, kind="stable")
    return np.asarray(values, np.uint64)[o], np.asarray(depths)[o]


def test_the_pairs_are_where_fast_runs():
    """every (k, m) of the range: the instance mgScanDiag counts is FAST exactly for PAIRS"""
    read = np.random.default_rng(0).integers(0, 4, 200).astype(np.uint8)
    bases, offs = util.concat_reads([read])
    fast = []
    with mg.knobs(SCAN_GENERIC=None, SCAN_DIV64=None, SCAN_PACKED_TEST=None):
        for k in KS:
            if k >= 32:
                continue
            for m in MS:
                sh = mg.seqhashCreate(k, 1 << m, SEED)
                before = util.scan_diag()
                mg.scan_batch(sh, bases, offs)
                since = util.scan_diag_since(before)
                assert len(since) == 1, (k, m, since)
                if ("batch", "FAST", 1) in since:
                    fast.append((k, m))
    assert fast == PAIRS


@pytest.mark.parametrize("k,m", PAIRS)
def test_both_tails_give_the_oracles_stream(k, m):
    d = 1 << m
    sh = mg.seqhashCreate(k, d, SEED)
    oh = po.Hasher(k, d, SEED)
    want = []
    for name, (bases, offs) in batches():
        ek, ep, ef, est = util.oracle_scan_batch(oh, bases, offs)
        oms = po.Modset(oh, BITS)
        for r in range(len(offs) - 1):
            oms.add_sequence(bases[offs[r]:offs[r + 1]])
        want.append((ek, ep, ef, est, set_pairs(oms.values()[1:oms.max + 1], oms.depths()[1:oms.max + 1])))
        oms.close()
    assert sum(len(w[0]) for w in want) >= 8980                                  # polyA alone: every start of it
    for knob in (1, 0):
        packed = knob == 1 and m <= 8
        one = [1, 0] if packed else [0, 1]
        with mg.knobs(SCAN_PACKED_TEST=knob, SCAN_GRID=1, SCAN_GENERIC=None, SCAN_DIV64=None):
            for (name, (bases, offs)), dr, (ek, ep, ef, est, (ev, ed)) in zip(batches(), dev_batches(), want):
                # positions and read ids
                b_scan, b_tail = util.scan_diag(), tails()
                km, pos, isf, st = mg.scan_batch(sh, bases, offs)
                since = util.scan_diag_since(b_scan)
                assert set(since) == {("batch", "FAST", 1)}, (name, knob, since)
                assert tails_since(b_tail) == [since[("batch", "FAST", 1)] * x for x in one], (name, knob)
                assert np.array_equal(st, est) and np.array_equal(km, ek) and np.array_equal(pos, ep) and np.array_equal(isf, ef), (name, knob)
                # the k-mers alone, through a set
                ms = mg.modsetCreate(sh, BITS)
                b_scan, b_tail = util.scan_diag(), tails()
                n = dr.add(ms)
                since = util.scan_diag_since(b_scan)
                assert set(since) == {("batch", "FAST", 0)}, (name, knob, since)
                assert tails_since(b_tail) == [since[("batch", "FAST", 0)] * x for x in one], (name, knob)
                assert n == len(ek), (name, knob)
                mg.check(mg.lib().modsetSyncToHost(ms, 1))
                v, dep, _ = mg.modset_arrays(ms)
                gv, gd = set_pairs(v[1:], dep[1:])
                assert np.array_equal(gv, ev) and np.array_equal(gd, ed), (name, knob)
                mg.lib().modsetDestroy(ms)
