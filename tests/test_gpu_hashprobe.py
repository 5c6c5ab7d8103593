"""The device arithmetic of modimizer_amd/csrc/mg_common.h, function by function, through the probe library (oracle/hash_probe.hip ->
oracle/libhashprobe.so: trivial kernels of its own around the header's __device__ functions, MgHashParams from the library's own
mgMakeParams) against Python / numpy INTEGER arithmetic: the scan's hit tests (mgDivisible, mgDivisibleOdd, mgDivisibleOdd32,
mgDivisibleAny32) against uint64 `%`, the reverse complements against a base-by-base loop, the table's hash against tests/util.py's
restatement (which tests/test_table_keys.py validates on the CPU).  Every comparison is exact.

The scan reaches these functions only with the hashes a batch happens to hold: a divisibility test that misfired once in d 10^6, only
above 2^38 or only for a large 2^24 mod d, would pass every comparison of whole scans.  Here each modulus gets the values where such a
test breaks: the multiples next to 2^24 j, to 2^32 and to the top of the range, with their neighbours."""
import ctypes as C
import os

import numpy as np
import pytest

import modimizer_amd as mg
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(ROOT, "oracle", "libhashprobe.so")
PROBE_SOURCES = ["hash_probe.hip", "../modimizer_amd/csrc/mg_common.h"]
PROBE_MARKER = "HASH_PROBE_HASH"

U = np.uint64
ANY64, ODD64, ODD32, ANY32 = range(4)                       # hashProbeDivisible's `which`
MIX_BITS, MIX_K, MIX_TOP, MIX_BUCKET, MIX_HOME = range(5)   # hashProbeMix's `what`
PARAMS = ("factor1", "mask", "k", "shift1", "d", "dShift", "dOddInv", "dOddLim", "c24", "inv32", "lim32", "small32")

# moduli past each limit of the 32-bit test and at the top of a U32, by their odd parts and shifts
BIG_D = [(1 << 15) - 1, (1 << 15) + 1, (1 << 16) - 1, (1 << 16) + 1, 3 << 13, 32767 * 2, 32767 << 16, 1 << 30, (1 << 31) - 1, 3 << 29]
SMALL_D = [3, 31, 97, 96, 1000]


def probe_source_hash():
    return util.probe_source_hash(PROBE_SOURCES)


def probe_binary_hash(path=None):
    return util.probe_binary_hash(path or PROBE_PATH, PROBE_MARKER)


def build_probe():
    return util.build_probe("libhashprobe.so", PROBE_MARKER, PROBE_SOURCES)


_probe = None


def probe():
    global _probe
    if _probe is None:
        mg.lib()                                         # first: the probe's libmodgpu.so IS the one the package has loaded
        P = C.CDLL(build_probe())
        P.hashProbeHash.restype = C.c_char_p
        if P.hashProbeHash().decode() != probe_source_hash():
            raise RuntimeError("libhashprobe.so (%s) is not the build of this tree's hash_probe.hip and mg_common.h (%s)"
                               % (P.hashProbeHash().decode(), probe_source_hash()))
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        for name, args in (("hashProbeParams", [i32, u32, vp]), ("hashProbeDivisible", [i32, i32, u32, vp, u64, vp]),
                           ("hashProbeDivisibleMany", [i32, i32, vp, u64, vp, u64, vp]), ("hashProbeRevComp16", [vp, u64, vp]),
                           ("hashProbeRevComp", [i32, vp, u64, vp]), ("hashProbeMix", [i32, i32, u32, vp, u64, vp])):
            f = getattr(P, name); f.restype = i32; f.argtypes = args
        _probe = P
    return _probe


def params(k, d):
    out = np.zeros(12, np.uint64)
    assert probe().hashProbeParams(k, d, out.ctypes.data) == 0
    return dict(zip(PARAMS, (int(x) for x in out)))


def divisible(which, k, ds, h):
    """h[len (ds), per] -> the device's answers, same shape, in ONE launch"""
    ds = np.ascontiguousarray(ds, np.uint32); h = np.ascontiguousarray(h, np.uint64)
    assert h.shape[0] == len(ds)
    out = np.full(h.shape, 7, np.uint8)
    rc = probe().hashProbeDivisibleMany(which, k, ds.ctypes.data, len(ds), h.ctypes.data, h.shape[1], out.ctypes.data)
    assert rc == 0, (rc, mg.lib().mgLastError())
    return out


def mix(what, b, arg, x):
    x = np.ascontiguousarray(x, np.uint64)
    out = np.zeros(len(x), np.uint64)
    rc = probe().hashProbeMix(what, b, arg, x.ctypes.data, len(x), out.ctypes.data)
    assert rc == 0, (rc, what, b, arg)
    return out


# ---- the values of h a modulus is tried on --------------------------------------------------------------------------------------

def h_set(ds, bits, rng):
    """for each modulus d of ds, the same 61 places of [0, 2^bits): 0, d, the top of the range; the largest multiple below 2^bits; the
    multiples nearest to 2^(bits - 16) j for j = 1, 255, 256, 65535 (2^24 j for 40-bit hashes: where mgDivisibleOdd32 splits h) and
    nearest to 2^32, each with both neighbours; the powers 2^24 and 2^32 and their neighbours; 16 random values; 16 random multiples"""
    d = np.asarray(ds, np.uint64)[:, None]
    top = U((1 << bits) - 1)
    one = U(1)
    cols = [np.zeros_like(d), d.copy(), np.full_like(d, top)]

    def around(m):
        m = np.where(m == 0, d, m)                             # (the multiple nearest to a place below d / 2 is 0: take d itself)
        m = np.where(m >= top, m - d, m)                       # (and one past the top of the range: the one before it)
        return [m - one, m, m + one]
    cols += around((top // d) * d)
    for j in (1, 255, 256, 65535):
        anchor = U(j << (bits - 16))
        cols += around(((anchor + d // U(2)) // d) * d)
    below = (U(1 << 32) // d) * d
    cols += around(below) + around(below + d)
    cols += [np.full_like(d, v) for v in ((1 << 24) - 1, 1 << 24, (1 << 32) - 1, 1 << 32, (1 << 32) + 1)]
    n = len(d)
    cols.append(rng.integers(0, 1 << bits, (n, 16), dtype=np.uint64))
    q = (rng.random((n, 16)) * (top // d + one).astype(np.float64)).astype(np.uint64)
    cols.append(np.minimum(q, top // d) * d)
    h = np.concatenate(cols, axis=1)
    assert h.max() <= top
    return np.ascontiguousarray(h)


def check_divisible(which, k, ds, seed):
    ds = np.asarray(ds, np.uint64)
    h = h_set(ds, 2 * k, np.random.default_rng(seed))
    want = (h % ds[:, None] == 0).astype(np.uint8)
    assert want[:, 1].all() and want[:, 4].all()                            # d and the largest multiple: the reference itself
    assert (want.sum(axis=1) >= 20).all() and ((1 - want).sum(axis=1) >= 10)[ds > 1].all()
    got = divisible(which, k, ds, h)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(ds[i]), int(h[i, j]), int(got[i, j])) for i, j in bad[:8]]
    return h.size


# ---- mgMakeParams ----------------------------------------------------------------------------------------------------------------

def test_params_against_their_definitions():
    """every odd dOdd below 2^15 and the moduli past each limit, at k = 20 and k = 21 (host arithmetic: runs without a device)"""
    for d in list(range(1, 1 << 15, 2)) + BIG_D + SMALL_D:
        shift = (d & -d).bit_length() - 1
        odd = d >> shift
        for k in (20, 21):
            p = params(k, d)
            assert (p["k"], p["shift1"], p["mask"], p["d"], p["dShift"]) == (k, 64 - 2 * k, (1 << (2 * k)) - 1, d, shift), (k, d)
            assert (odd * p["dOddInv"]) % (1 << 64) == 1, (k, d)
            assert p["dOddLim"] == ((1 << 64) - 1) // odd, (k, d)
            assert p["c24"] == (1 << 24) % odd and p["lim32"] == ((1 << 32) - 1) // odd, (k, d)
            assert p["inv32"] == p["dOddInv"] % (1 << 32) and (odd * p["inv32"]) % (1 << 32) == 1, (k, d)
            assert p["small32"] == (1 if 2 * k <= 40 and odd < (1 << 15) else 0), (k, d)
    assert probe().hashProbeParams(0, 3, None) == -1 and probe().hashProbeParams(32, 3, None) == -1 and probe().hashProbeParams(20, 0, None) == -1


# ---- the four hit tests ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_odd32_every_modulus_at_40_bits():
    """mgDivisibleOdd32 at k = 20 for all 16384 odd moduli below 2^15: about a million evaluations in one launch"""
    n = check_divisible(ODD32, 20, np.arange(1, 1 << 15, 2), 20)
    assert n == 16384 * 61


@pytest.mark.gpu
def test_any32_shifts_up_to_16():
    """mgDivisibleAny32 at k = 20: odd parts 3, 32765, 32767 times 2^1, 2^5, 2^13 and 2^16.  With 2^16 the modulus itself is far above
    2^15 (32767 2^16 is nearly 2^31) and the library still takes the 32-bit test: what counts is the odd part, h >> dShift being below
    2^40 all the more"""
    ds = [odd << s for odd in (3, 32765, 32767) for s in (1, 5, 13, 16)]
    for d in ds:
        assert params(20, d)["small32"] == 1
    check_divisible(ANY32, 20, ds, 21)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31])
def test_any64_and_odd64(k):
    """mgDivisible on every modulus of the lists, mgDivisibleOdd on the odd ones, at 42- and 62-bit hashes"""
    ds = BIG_D + SMALL_D
    check_divisible(ANY64, k, ds, k)
    check_divisible(ODD64, k, [d for d in ds if d & 1], k + 100)
    # and at k = 20 next to the 32-bit tests, on the moduli those take: the two must agree wherever both apply
    check_divisible(ANY64, 20, [3, 32767, 6, 24576, 65534, 32767 << 16], k + 200)


@pytest.mark.gpu
def test_refused_what_the_library_never_runs():
    P = probe()
    h = np.zeros(4, np.uint64); out = np.zeros(4, np.uint8)
    call = lambda which, k, d: P.hashProbeDivisible(which, k, d, h.ctypes.data, 4, out.ctypes.data)
    assert call(ODD32, 21, 3) == -1 and call(ANY32, 21, 6) == -1                    # small32 == 0: 42-bit hashes
    assert call(ODD32, 20, 32769) == -1 and call(ANY32, 20, 65538) == -1            # small32 == 0: the odd part
    assert call(ODD32, 20, 6) == -1 and call(ODD64, 21, 6) == -1                    # odd tests on an even modulus
    assert call(ODD32, 20, 3) == 0 and call(ANY32, 20, 6) == 0 and call(ODD64, 21, 3) == 0 and call(ANY64, 21, 6) == 0
    assert out.all()                                                                # 0 is a multiple of everything
    h[0] = 1 << 40
    assert call(ODD32, 20, 3) == -1                                                 # not a 40-bit hash


# ---- reverse complements ---------------------------------------------------------------------------------------------------------

def revcomp_ref(x, k):
    """base by base: base i of the result is the complement of base k - 1 - i"""
    x = np.asarray(x, np.uint64)
    out = np.zeros_like(x)
    for i in range(k):
        out |= (U(3) - ((x >> U(2 * i)) & U(3))) << U(2 * (k - 1 - i))
    return out


@pytest.mark.gpu
def test_revcomp16():
    rng = np.random.default_rng(16)
    x = np.concatenate([rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAA], np.uint32), (U(1) << np.arange(32, dtype=np.uint64)).astype(np.uint32)])
    out = np.zeros_like(x); back = np.zeros_like(x)
    assert probe().hashProbeRevComp16(x.ctypes.data, len(x), out.ctypes.data) == 0
    assert np.array_equal(out, revcomp_ref(x.astype(np.uint64), 16).astype(np.uint32))
    assert probe().hashProbeRevComp16(out.ctypes.data, len(x), back.ctypes.data) == 0
    assert np.array_equal(back, x)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 32))
def test_revcomp_every_k(k):
    rng = np.random.default_rng(k)
    mask = (1 << (2 * k)) - 1
    x = np.concatenate([rng.integers(0, mask + 1, 4096, dtype=np.uint64), np.array([0, mask, 1, 1 << (2 * k - 1), mask >> 1, mask - 1], np.uint64),
                        U(1) << np.arange(2 * k, dtype=np.uint64)])
    out = np.zeros_like(x); back = np.zeros_like(x)
    assert probe().hashProbeRevComp(k, x.ctypes.data, len(x), out.ctypes.data) == 0
    assert np.array_equal(out, revcomp_ref(x, k))
    assert probe().hashProbeRevComp(k, out.ctypes.data, len(x), back.ctypes.data) == 0            # the other direction: an involution
    assert np.array_equal(back, x)


# ---- the table's hash --------------------------------------------------------------------------------------------------------------

def mix_values(b, rng, n_random=1 << 18):
    if b <= 20:
        return np.arange(1 << b, dtype=np.uint64)
    top = 1 << b
    return np.concatenate([rng.integers(0, top, n_random, dtype=np.uint64), np.arange(4096, dtype=np.uint64), np.arange(top - 4096, top, dtype=np.uint64)])


@pytest.mark.gpu
@pytest.mark.parametrize("b", range(2, 64, 2))
def test_mix_bits_and_mix_k(b):
    """mgMixBits (its 32-bit branch up to b = 32) and mgMixK (the cheap top bits from b = 24) equal tests/util.py's; over every b-bit value
    up to b = 20, where each must be a bijection"""
    x = mix_values(b, np.random.default_rng(b))
    for what, ref in ((MIX_BITS, util.mix_bits), (MIX_K, util.mix_k)):
        got = mix(what, b, 0, x)
        assert np.array_equal(got, ref(x, b)), (what, b)
        assert int(got.max()) < (1 << b)
        if b <= 20:
            assert np.array_equal(np.sort(got), x), (what, b, "not a bijection")


@pytest.mark.gpu
@pytest.mark.parametrize("b", [24, 30, 40, 42, 44, 54, 62])
def test_mix_top_of_kmer(b):
    """the scan's shortcut to the first partition digit: the top hiB bits of the mix from the k-mer itself (b = 42: the low part crosses 32 bits)"""
    x = mix_values(b, np.random.default_rng(b), 1 << 16)
    full = util.mix_k(x, b)
    for hib in range(1, 11):
        assert np.array_equal(mix(MIX_TOP, b, hib, x), full >> U(b - hib)), (b, hib)


@pytest.mark.gpu
@pytest.mark.parametrize("kbits", [2, 6, 8, 24, 42, 62])
def test_bucket_of(kbits):
    """mgBucketOfM over the k-mer's mix, including tables with more buckets than there are k-mers (kbits < log2NB: the mix shifted UP)"""
    x = mix_values(kbits, np.random.default_rng(kbits), 1 << 16)
    m = util.mix_k(x, kbits)
    for log2nb in (0, 4, 8, 12, 20):
        got = mix(MIX_BUCKET, kbits, log2nb, x)
        assert np.array_equal(got, util.bucket_of(x, kbits // 2, log2nb)), (kbits, log2nb)
        plain = np.zeros_like(m) if not log2nb else (m >> U(kbits - log2nb) if kbits >= log2nb else m << U(log2nb - kbits))   # the definition
        assert np.array_equal(got, plain) and int(got.max()) < (1 << log2nb), (kbits, log2nb)


@pytest.mark.gpu
@pytest.mark.parametrize("kbits", [22, 24, 62])
def test_home_of(kbits):
    x = mix_values(kbits, np.random.default_rng(kbits), 1 << 16)
    for r in (64, 192, 256, 2368, 4096):
        got = mix(MIX_HOME, kbits, r, x)
        assert int(got.max()) < r
        assert np.array_equal(got, util.home_of(x, kbits // 2, r)), (kbits, r)


@pytest.mark.gpu
def test_mix_refuses_what_no_kernel_passes():
    P = probe()
    x = np.array([1 << 24], np.uint64); out = np.zeros(1, np.uint64)
    call = lambda what, b, arg: P.hashProbeMix(what, b, arg, x.ctypes.data, 1, out.ctypes.data)
    assert call(MIX_K, 24, 0) == -1                       # a value of more than b bits
    assert call(MIX_TOP, 22, 4) == -1 and call(MIX_TOP, 26, 0) == -1 and call(MIX_TOP, 26, 11) == -1 and call(MIX_HOME, 26, 0) == -1
    assert call(MIX_K, 26, 0) == 0 and int(out[0]) == int(util.mix_k(x, 26)[0])
