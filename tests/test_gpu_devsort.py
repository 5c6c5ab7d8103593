"""modimizer_amd/csrc/mg_devsort.hip as primitives: mgExclusiveScan, mgRefStableSort and mgKeyBits, driven through the probe library
(oracle/devsort_probe.hip -> oracle/libdevsortprobe.so, which is LINKED against libmodgpu.so: the code that runs is the library's own)
and held against numpy.  The five call sites (loc[] / rev[] of the Reference, the inverse lists of modasm's ingest, the neighbour pass of
-C, the two sorts of -P) reach them only with what their data happens to be; here the inputs are the edges: 1, 2, 3 and 4 sort passes
with and without values, keys that differ in one byte only, equal keys in every wave segment of every tile, waves of one digit, 0 next
to 255, a ragged last round of zeros, one key a million times over; scans in place and not, n around the multiples of 4096, sums of
exactly 2^32 - 1, more than 1024 and 2048 tiles.  Integers only: every comparison is exact.

MG_SCAN_TILE and MG_RSORT_TILE are plain data (no GPU, no library needed to import this module): tests/test_abi.py asserts that they
are the header's, and the other test files take them from here."""
import ctypes as C
import os

import numpy as np
import pytest

import modimizer_amd as mg
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
PROBE_PATH = os.path.join(ORACLE, "libdevsortprobe.so")

MG_SCAN_TILE = 4096            # mg_devsort.h: elements per workgroup of a scan pass
MG_RSORT_TILE = 8192           # mg_devsort.h: elements per workgroup of a sort pass; a wave takes a quarter of it, 64 at a time
WAVE_PART = MG_RSORT_TILE // 4

GUARD = 8
FENCE = np.uint32(0xDEADBEEF)
SCAN_LENGTHS = [0, 1, 15, 16, 17, 255, 256, 4095, 4096, 4097, 8191, 8193, 4096 * 1024 - 1, 4096 * 1024 + 1, 4096 * 2048 + 1]
KEY_BITS = [1, 7, 8, 9, 16, 17, 24, 25, 31, 32]
SORT_LENGTHS = [1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 100]


# ---- the probe ----------------------------------------------------------------------------------

PROBE_SOURCES = ["devsort_probe.hip", "../modimizer_amd/csrc/mg_devsort.h", "../modimizer_amd/csrc/mg_common.h"]
PROBE_MARKER = "DEVSORT_PROBE_HASH"


def probe_source_hash():
    """the hash oracle/Makefile bakes into the probe, over its three sources"""
    return util.probe_source_hash(PROBE_SOURCES)


def probe_binary_hash(path=None):
    """the hash a built probe carries, read out of the file (no dlopen); None if there is no such file or marker"""
    return util.probe_binary_hash(path or PROBE_PATH, PROBE_MARKER)


def build_probe():
    """make the probe if the one in the tree is not the build of the tree's sources"""
    return util.build_probe("libdevsortprobe.so", PROBE_MARKER, PROBE_SOURCES)


_probe = None


def probe():
    global _probe
    if _probe is None:
        mg.lib()                                         # first: the probe's libmodgpu.so IS the one the package has loaded
        P = C.CDLL(build_probe())
        P.devsortProbeHash.restype = C.c_char_p
        if P.devsortProbeHash().decode() != probe_source_hash():
            raise RuntimeError("libdevsortprobe.so (%s) is not the build of this tree's devsort_probe.hip, mg_devsort.h and mg_common.h (%s)"
                               % (P.devsortProbeHash().decode(), probe_source_hash()))
        P.devsortProbeKeyBits.restype = C.c_int
        P.devsortProbeKeyBits.argtypes = [C.c_uint64]
        P.devsortProbeScratchWords.restype = C.c_uint64
        P.devsortProbeScratchWords.argtypes = [C.c_uint64]
        P.devsortProbeScan.restype = C.c_int
        P.devsortProbeScan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
        P.devsortProbeSort.restype = C.c_int
        P.devsortProbeSort.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _probe = P
    return _probe


@pytest.mark.gpu
def test_probe_is_the_build_of_this_tree():
    P = probe()
    assert P.devsortProbeHash().decode() == probe_source_hash() == probe_binary_hash()


# ---- mgKeyBits ----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_key_bits():
    """the bits of the keys 0 .. maxKey, at least 1 and at most 32: the table around every pass boundary, and for random m the sort
    by that many bits sees every key up to m.  (No kernel runs; the probe loads the HIP library.)"""
    P = probe()
    table = {0: 1, 1: 1, 2: 2, 3: 2, 255: 8, 256: 9, 65535: 16, 65536: 17, (1 << 24) - 1: 24, 1 << 24: 25, (1 << 32) - 1: 32,
             1 << 32: 32, 1 << 40: 32}
    got = {m: P.devsortProbeKeyBits(m) for m in table}
    assert got == table
    rng = np.random.default_rng(32)
    ms = [int(m) for m in rng.integers(0, 1 << 32, 300)] + [int(1 << b) + d for b in range(1, 32) for d in (-1, 0, 1)]
    for m in ms:
        b = P.devsortProbeKeyBits(m)
        assert 1 <= b <= 32 and m < 1 << b, (m, b)
        assert b == 1 or m >= 1 << (b - 1), (m, b, "more bits than the keys have: a pass too many is not wrong, but it is not what the header says")


# ---- mgExclusiveScan ----------------------------------------------------------------------------

def scan_inputs(n):
    """(name, x) for a length; every generator is seeded by n"""
    rng = np.random.default_rng(4096 + n)
    cases = [("counts 0 .. 3", rng.integers(0, 4, n).astype(np.uint32)),
             ("all ones", np.ones(n, np.uint32)),
             ("random, full width", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))]      # the sums wrap: numpy's uint32 wraps the same way
    x = np.zeros(n, np.uint32)                           # seven non-zeros, none in the first tile where there is a second
    lo = MG_SCAN_TILE if n > MG_SCAN_TILE + 7 else 1
    if n > lo:
        at = lo + (rng.choice(n - lo, min(7, n - lo), replace=False) if n - lo < 10000 else rng.permutation(np.unique(rng.integers(0, n - lo, 40)))[:7])      # anywhere behind the first tile, the last tiles too
        assert len(at) == min(7, n - lo)
        x[at] = rng.integers(1, 1000, len(at)).astype(np.uint32)
    cases.append(("mostly zeros, the first tile empty", x))
    for p in (0, 4095, 4096):                            # the sum is 2^32 - 1 exactly from p on: nothing may wrap
        if p < n:
            x = np.zeros(n, np.uint32); x[p] = 0xFFFFFFFF
            cases.append(("0xFFFFFFFF at %d, zeros" % p, x))
    return cases


def run_scan(name, x, want, want_total, in_place, with_total):
    """one probe call; asserts everything that is to hold of it"""
    P = probe()
    n = len(x)
    buf = np.full(n + 2 * GUARD, FENCE, np.uint32)
    buf[GUARD:GUARD + n] = x if in_place else np.uint32(0x5A5A5A5A)
    xin = x.copy()
    total = C.c_uint32(0xA5A5A5A5)
    what = (name, "n %d" % n, "in place" if in_place else "distinct buffers", "with total" if with_total else "no total")
    assert P.devsortProbeScan(xin.ctypes.data, buf.ctypes.data, n, GUARD, int(in_place), int(with_total), C.byref(total)) == 0, what
    got = buf[GUARD:GUARD + n]
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(what + ("%d wrong, first at %d (tile %d): %#x, not %#x" % (len(bad), bad[0], bad[0] // MG_SCAN_TILE, int(got[bad[0]]), int(want[bad[0]])),))
    assert np.all(buf[:GUARD] == FENCE) and np.all(buf[GUARD + n:] == FENCE), what + ("words outside out[0 .. n) were written",)
    assert np.array_equal(xin, x), what + ("in[] was changed",)
    assert total.value == (want_total if with_total else 0xA5A5A5A5), what + ("total %#x, not %#x" % (total.value, want_total),)
    if n == 0:
        assert len(buf) == 2 * GUARD and want_total == 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_LENGTHS)
def test_exclusive_scan(n):
    """out[i] = in[0] + ... + in[i - 1] modulo 2^32 and the total on the host, nothing else written, in[] as it was: distinct buffers
    and in place, with and without the total.  n == 0: *total = 0 and nothing happens.  The scratch a caller is told to expect holds
    what the scan writes: a word per tile and the total behind them."""
    P = probe()
    tiles = (n + MG_SCAN_TILE - 1) // MG_SCAN_TILE
    assert P.devsortProbeScratchWords(n) >= tiles + 1
    for name, x in scan_inputs(n):
        inc = np.cumsum(x, dtype=np.uint32)
        want = np.concatenate([np.zeros(1, np.uint32), inc[:-1]]) if n else np.zeros(0, np.uint32)
        want_total = int(inc[-1]) if n else 0
        if "0xFFFFFFFF at" in name:
            assert want_total == 0xFFFFFFFF and int(x.astype(np.uint64).sum()) == 0xFFFFFFFF
        for in_place in (False, True):
            for with_total in (False, True):
                run_scan(name, x, want, want_total, in_place, with_total)


# ---- mgRefStableSort ----------------------------------------------------------------------------

def passes_of(key_bits):
    return max((key_bits + 7) // 8, 1)


def draw_vals(rng, n):
    """arbitrary words with duplicates, not a permutation: a value written twice cannot pass as a reordering"""
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    m = n // 8
    if m:
        v[rng.choice(n, m, replace=False)] = v[rng.choice(n, m, replace=False)]
    return v


def run_sort(name, keys, vals, key_bits):
    """one probe call against np.argsort (kind="stable") of the bits the passes look at; asserts everything that is to hold of it"""
    P = probe()
    n = len(keys)
    assert n > 0 and keys.dtype == np.uint32 and (vals is None or (vals.dtype == np.uint32 and len(vals) == n))
    passes = passes_of(key_bits)
    seen = keys & np.uint32((1 << (8 * passes)) - 1)
    order = np.argsort(seen, kind="stable")
    src = np.arange(n, dtype=np.uint32) if vals is None else vals
    want = src[order]
    out = np.full(n, 0xA5A5A5A5, np.uint32)
    keys_in, keys_back = keys.copy(), np.zeros(n, np.uint32)
    vals_in, vals_back = (None, None) if vals is None else (vals.copy(), np.zeros(n, np.uint32))
    what = (name, "n %d" % n, "keyBits %d: %d passes" % (key_bits, passes), "positions" if vals is None else "vals")
    rc = P.devsortProbeSort(keys_in.ctypes.data, None if vals is None else vals_in.ctypes.data, n, key_bits, out.ctypes.data,
                            keys_back.ctypes.data, None if vals is None else vals_back.ctypes.data)
    assert rc == 0, what
    assert np.array_equal(keys_in, keys) and np.array_equal(keys_back, keys), what + ("the input keys were changed",)
    if vals is not None:
        assert np.array_equal(vals_in, vals) and np.array_equal(vals_back, vals), what + ("the input vals were changed",)
    is_permutation = np.array_equal(np.sort(out), np.sort(want))      # of the expected multiset: nothing written twice, nothing lost
    if not np.array_equal(out, want):
        j = int(np.flatnonzero(out != want)[0])
        there = np.flatnonzero(src == out[j])            # where the value that came out instead sits in the input
        if len(there) == 0:
            kind = "%#x is no input value" % int(out[j])
        elif np.any(seen[there] == seen[order[j]]):
            kind = "a STABILITY fault: the element that came instead has the same key %#x" % int(seen[order[j]])
        else:
            kind = "an ORDERING fault: key %#x came where key %#x belongs" % (int(seen[there[0]]), int(seen[order[j]]))
        multiset = "a permutation of the expected values" if is_permutation else "NOT a permutation of the expected values"
        raise AssertionError(what + ("%d wrong, first at %d (input place %d: tile %d, wave %d, round %d, lane %d): %#x, not %#x"
                                     % (int((out != want).sum()), j, order[j], order[j] // MG_RSORT_TILE, order[j] % MG_RSORT_TILE // WAVE_PART,
                                        order[j] % WAVE_PART // 64, order[j] % 64, int(out[j]), int(want[j])), kind, multiset))
    assert is_permutation, what


def both(name, keys, key_bits, rng):
    """with values of its own and with the positions (vals == 0: the FIRST kernel on pass 0, the other one afterwards)"""
    run_sort(name, keys, draw_vals(rng, len(keys)), key_bits)
    run_sort(name, keys, None, key_bits)


def uniform_keys(rng, n, bits):
    return rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("key_bits", KEY_BITS)
def test_sort_key_widths(key_bits):
    """1, 2, 3 and 4 passes (the fourth is the one that writes the second key array a second time), lengths around the wave round, the
    wave's part of a tile and the tile: keys uniform below 2^keyBits; keys that differ in the top digit only and in the bottom digit
    only (a pass that is dropped, or that reads the wrong array, leaves them unsorted or unstable); and bits above the last pass's
    digit, which the sort does not look at"""
    passes = passes_of(key_bits)
    top_shift = 8 * (passes - 1)
    for n in SORT_LENGTHS:
        rng = np.random.default_rng(1000 * key_bits + n)
        both("uniform", uniform_keys(rng, n, key_bits), key_bits, rng)
        if key_bits > 8:
            low = np.uint32(0x5A5A5A & ((1 << top_shift) - 1))
            both("the top digit only", (uniform_keys(rng, n, key_bits - top_shift) << np.uint32(top_shift)) | low, key_bits, rng)
            high = np.uint32(((1 << key_bits) - 1) & 0xA5A5A500)
            both("the bottom digit only", uniform_keys(rng, n, 8) | high, key_bits, rng)
        if passes < 4:
            junk = uniform_keys(rng, n, 32 - 8 * passes) << np.uint32(8 * passes)
            both("uniform, with bits above the last digit", uniform_keys(rng, n, key_bits) | junk, key_bits, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2, 3, 4])
@pytest.mark.parametrize("distinct", [2, 3, 256])
def test_sort_is_stable_across_waves_and_tiles(distinct, passes):
    """few distinct keys over six tiles and a ragged seventh: every key occurs in every wave's part of every tile, so its occurrences have
    to come out in input order across the 64-, 2048- and 8192-element lines"""
    n = 5 * MG_RSORT_TILE + WAVE_PART + 37
    rng = np.random.default_rng(100 * distinct + passes)
    values = np.zeros(0, np.uint32)
    while len(values) < distinct:                        # (all 256 of them where there is one byte)
        values = np.unique(np.concatenate([values, uniform_keys(rng, distinct, 8 * passes)]))
    values = rng.permutation(values)[:distinct]
    keys = values[rng.integers(0, distinct, n)]
    parts = np.arange(n) // WAVE_PART
    if distinct <= 3:
        assert all(len(np.unique(parts[keys == v])) == parts[-1] + 1 for v in values)
    both("%d distinct keys" % distinct, keys, 8 * passes, rng)


def wave_cases():
    """(name, keys, keyBits): what the ballots and the counter of a wave round have to get right"""
    rng = np.random.default_rng(64)
    n = MG_RSORT_TILE + WAVE_PART + 65
    i = np.arange(n, dtype=np.uint32)
    cases = [("all keys 0", np.zeros(n, np.uint32), 8), ("all keys 0, 4 passes", np.zeros(n, np.uint32), 32),
             ("all keys 255", np.full(n, 255, np.uint32), 8), ("all keys 0xFFFFFFFF", np.full(n, 0xFFFFFFFF, np.uint32), 32),
             ("0 and 255 alternating", (i & 1) * np.uint32(255), 8), ("255 and 0 alternating", (1 - (i & 1)) * np.uint32(255), 8),
             ("0 and 255 in every byte, alternating", (i & 1) * np.uint32(0xFFFFFFFF), 32)]
    digit = ((i // 64) * 37 + 11) % 256                  # one digit per round of 64, another one in the next round
    cases += [("one digit per wave round", digit.astype(np.uint32), 8),
              ("one digit per wave round, in every byte", digit.astype(np.uint32) * np.uint32(0x01010101), 32)]
    # a ragged last round whose live keys are all 0 (the dead lanes hold digit 0 too), zeros earlier as well
    for k in (0, 5, 31, 32, 70):                         # the last round: the tile's first, some round, wave 0's last, wave 1's first, in wave 2
        for r in (1, 31, 33, 63):
            m = MG_RSORT_TILE + 64 * k + r
            for bits in (8, 16):
                keys = uniform_keys(rng, m, bits)
                keys[100:300] = 0
                keys[MG_RSORT_TILE:MG_RSORT_TILE + 40] = 0
                keys[m - r:] = 0
                cases.append(("a last round of %d zeros after %d full rounds" % (r, k), keys, bits))
    return cases


@pytest.mark.gpu
def test_sort_wave_matching():
    """every lane finds its peers by eight ballots, and the first peer moves the wave's counter on: waves whose 64 lanes hold one digit,
    digits 0 and 255 side by side, a digit that changes from round to round, and a ragged last round of zeros"""
    rng = np.random.default_rng(65)
    for name, keys, bits in wave_cases():
        both(name, keys, bits, rng)


@pytest.mark.gpu
def test_sort_skewed_keys():
    """one key 2^20 times over and 1000 others scattered among them sort like any other input (3 passes)"""
    rng = np.random.default_rng(20)
    n = (1 << 20) + 1000
    keys = np.full(n, 0x123456, np.uint32)
    at = rng.choice(n, 1000, replace=False)
    keys[at] = uniform_keys(rng, 1000, 24)
    both("skew", keys, 24, rng)


@pytest.mark.gpu
def test_sort_four_passes_of_positions():
    """2^21 + 5 keys of 32 random bits, vals == 0: 257 tiles, four passes, the positions as values"""
    rng = np.random.default_rng(21)
    n = (1 << 21) + 5
    run_sort("random, full width", uniform_keys(rng, n, 32), None, 32)
