"""CPU: the tests' own restatement of the device table's hash and geometry (tests/util.py) and the k-mers crafted with it.  The GPU
tests lean on these to crowd one bucket; a mistake here would make them test nothing, so the generator is checked where no GPU is."""
import numpy as np
import pytest

import util


@pytest.mark.parametrize("bits", [24, 30, 36, 42, 54, 62])
def test_mix_is_a_bijection_on_a_sample(bits):
    rng = np.random.default_rng(bits)
    n = 1 << 20
    x = np.unique(np.concatenate([rng.integers(0, 1 << bits, n, dtype=np.uint64),
                                  np.arange(4096, dtype=np.uint64), np.uint64((1 << bits) - 1) - np.arange(4096, dtype=np.uint64)]))
    m = util.mix_k(x, bits)
    assert m.dtype == np.uint64 and int(m.max()) < (1 << bits)
    assert len(np.unique(m)) == len(x), "two k-mers with one table hash"
    assert not np.array_equal(m, x)


def test_mix_is_a_bijection_of_all_24_bit_values():
    x = np.arange(1 << 24, dtype=np.uint64)
    seen = np.zeros(1 << 24, bool)
    seen[util.mix_k(x, 24)] = True
    assert seen.all()


def test_mix_below_24_bits_is_the_plain_one():
    x = np.arange(1 << 22, dtype=np.uint64)
    assert np.array_equal(util.mix_k(x, 22), util.mix_bits(x, 22))
    assert len(np.unique(util.mix_bits(x, 22))) == len(x)


@pytest.mark.parametrize("k,prefix,prefix_bits", [(12, 0, 10), (15, 1023, 10), (21, 0, 10), (21, 5, 4), (21, 1, 1), (22, 77, 9), (27, 311, 10),
                                                  (31, 3, 5), (21, 0, 0)])
def test_crafted_kmers_carry_their_prefix(k, prefix, prefix_bits):
    rng = np.random.default_rng(k * 1000 + prefix)
    n = 2000 if k == 12 else 20_000
    km = util.kmers_with_mix_prefix(rng, n, prefix, prefix_bits, k)
    assert km.dtype == np.uint64 and len(km) == n
    assert len(np.unique(km)) == n, "not distinct"
    assert int(km.max()) < (1 << (2 * k)), "not a k-mer"
    m = util.mix_k(km, 2 * k)
    assert (m >> np.uint64(2 * k - prefix_bits) == prefix).all() if prefix_bits else True
    # every table of up to 2^prefix_bits buckets has them in one bucket, a larger one spreads them
    for lg in range(0, prefix_bits + 1):
        assert len(np.unique(util.bucket_of(km, k, lg))) == 1
    if prefix_bits < 10 and k > 12:
        assert len(np.unique(util.bucket_of(km, k, prefix_bits + 2))) == 4


def test_geometry_of_the_worked_cases():
    """the geometries the skew tests are built on (default bucket size, and 256 slots a bucket)"""
    assert util.table_geometry(util.slots_for(30_000, 60, 22)) == (4, 4096)
    assert util.table_geometry(util.slots_for(30_000, 40, 22)) == (5, 2368)
    assert util.table_geometry(util.slots_for(90_000, 60, 22)) == (6, 2368)
    assert util.table_geometry(util.slots_for(39_000, 60, 22), 256) == (8, 256)
    assert util.table_geometry(util.slots_for(39_000, 40, 22), 256) == (9, 192)
    assert util.table_geometry(util.slots_for(200_000, 40, 22), 256) == (11, 256)
    assert util.table_geometry(util.slots_for(100_000, 40, 22), 256) == (10, 256)
