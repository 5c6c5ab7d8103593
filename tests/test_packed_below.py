"""The scan filter's packed threshold test on the host: mgScanBytesBelow (acc, nRep) is the line the kernel compiles
(csrc/mg_packedtest.h), bit 8j + 7 set for the bytes of acc below N where nRep = 0x01010101 N.

The only way one byte's answer can depend on another is the borrow of the word-wide subtraction, which runs from a byte into the one
above it.  So: every pair of adjacent bytes (65 536 of them), in byte lanes (0, 1), (1, 2) and (2, 3), the other two lanes all ones
and all zeros, for every N the filter can have (d = 8 .. 256: N = 32 .. 1).  A byte below N is always flagged -- a miss would lose a
modimizer.  A flagged byte that is not below N equals N and sits directly above a flagged byte -- such a start costs the exact
evaluation a slot and nothing else; the test also sees that this happens, so that it is not vacuous."""
import numpy as np
import pytest

import modimizer_amd as mg

NS = [1, 2, 4, 8, 16, 32]
TOPS = 0x80808080


def words():
    """every adjacent pair at every place, over both fills"""
    lo, hi = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(256, dtype=np.uint64))
    pair = (lo | (hi << np.uint64(8))).reshape(-1)
    out = []
    for place in range(3):
        keep = np.uint64(0xffffffff ^ (0xffff << (8 * place)))
        for fill in (np.uint64(0xffffffff), np.uint64(0)):
            out.append((fill & keep) | (pair << np.uint64(8 * place)))
    return np.concatenate(out).astype(np.uint32)


def test_hook_is_declared_and_bound():
    assert "mgScanBytesBelow" in mg.EXPORTS and "mgScanTailDiag" in mg.EXPORTS
    assert mg.lib().mgScanBytesBelow(0x03040005, 0x04040404) == 0x80808000       # 0 and 3 are below 4, 5 is not; the 4 directly above the flagged 0 is passed too


@pytest.mark.parametrize("n", NS)
def test_bytes_below(n):
    f = mg.lib().mgScanBytesBelow
    w = words()
    assert len(w) == 6 * 65536
    rep = 0x01010101 * n
    flags = np.fromiter((f(x, rep) for x in w.tolist()), np.uint32, len(w))
    assert not (flags & np.uint32(~TOPS & 0xffffffff)).any()
    byte = [(w >> np.uint32(8 * j)) & np.uint32(0xff) for j in range(4)]
    flag = [((flags >> np.uint32(8 * j + 7)) & np.uint32(1)).astype(bool) for j in range(4)]
    extra = 0
    for j in range(4):
        below = byte[j] < n
        assert flag[j][below].all(), (n, j)                                      # no false negative
        more = flag[j] & ~below
        if j == 0:
            assert not more.any(), n                                             # nothing below the lowest byte can borrow
        else:
            assert (byte[j][more] == n).all() and flag[j - 1][more].all(), (n, j)
        extra += int(more.sum())
    assert extra > 0, n
