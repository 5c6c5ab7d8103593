"""Shared by tests/test_gpu_modutils_x.py and tests/test_gpu_modutils_copy.py: the goldens of make_golden_tenx.py, the 10x trim restated
in numpy, and the expected set from the CPU oracle."""
import ctypes as C
import gzip
import os

import numpy as np

import modimizer_amd as mg
import util
from oracle import pyoracle as po

TAGS = {"k11w4": (20, 11, 4, 17), "k25w3": (20, 25, 3, 17)}      # make_golden_tenx.TAGS
COPY, COPY_M = (2, 3, 6), 5                                       # its -s and -sM thresholds
SKIP = 23
_CODE = np.full(256, 255, np.uint8)
for _c, _v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("N", 0)):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _v


def gpath(name):
    return os.path.join(util.GOLDEN, name)


def golden_lines(tag, ext):
    """(the added line, [summary after -x, after -s, after -sM]) of the golden run's stdout"""
    lines = util.golden_text("tenx_%s_%s.stdout.txt" % (tag, ext)).splitlines(keepends=True)
    assert len(lines) == 11 and lines[1].startswith("added ")
    return lines[1], ["".join(lines[2 + 3 * i:5 + 3 * i]) for i in range(3)]


def golden_mod(tag, ext):
    """the golden .mod's bytes (modsetWrite's layout) and its arrays: max, value[], depth[], info[] (entries 0 .. max)"""
    raw = gzip.open(gpath("tenx_%s_%s.mod" % (tag, ext))).read()
    bits, n = np.frombuffer(raw, np.int32, 1, 8)[0], np.frombuffer(raw, np.uint32, 1, 12)[0]
    at = 16 + 8 + C.sizeof(mg.Seqhash) + 4 * (1 << int(bits))
    value = np.frombuffer(raw, np.uint64, n, at); at += 8 * int(n)
    depth = np.frombuffer(raw, np.uint16, n, at); at += 2 * int(n)
    info = np.frombuffer(raw, np.uint8, n, at)
    assert at + int(n) == len(raw)
    return raw, int(n) - 1, value, depth, info


def file_reads(text):
    """the records of FASTA / FASTQ text as the readers deliver them: uint8 arrays of 0 .. 3 (N is 0; FASTA drops what is no base)"""
    lines = text.split(b"\n")
    if text[:1] == b"@":
        return [_CODE[np.frombuffer(lines[i], np.uint8)] for i in range(1, len(lines) - 1, 4)]
    recs = []
    for l in lines:
        if l[:1] == b">":
            recs.append([])
        elif l:
            c = _CODE[np.frombuffer(l, np.uint8)]
            recs[-1].append(c[c < 4])
    return [np.concatenate(r) if r else np.zeros(0, np.uint8) for r in recs]


def trim(reads, first=1):
    """modutils.c:44: the record with an odd number loses its first 23 bases (a shorter one all it has)"""
    return [r[SKIP:] if (first + i) & 1 else r for i, r in enumerate(reads)]


def oracle_set(tag_or_params, batches):
    """the CPU oracle's set after adding every read of every batch, in order, and the hashes each batch gave"""
    B, k, w, s = TAGS[tag_or_params] if isinstance(tag_or_params, str) else tag_or_params
    oms = po.Modset(po.Hasher(k, w, s), B)
    return oms, [sum(int(oms.add_sequence(r)) for r in reads) for reads in batches]


def new_set(tag):
    B, k, w, s = TAGS[tag]
    return mg.modsetCreate(mg.seqhashCreate(k, w, s), B)


def destroy(ms):
    L = mg.lib()
    sh = C.cast(ms.contents.hasher, C.c_void_p).value
    L.modsetDestroy(ms)
    L.mgSeqhashDestroy(C.cast(sh, C.POINTER(mg.Seqhash)))


def chain(depth, c1, c2, cm):
    """modutils.c:209-212, the else-if chain as it stands"""
    d = depth.astype(np.int64)
    return np.where(d < c1, 0, np.where(d < c2, 1, np.where(d < cm, 2, 3))).astype(np.uint8)


def host_views(ms):
    """the host arrays themselves: depth[0 .. max], info[0 .. max]"""
    n = ms.contents.max + 1
    return np.ctypeslib.as_array(ms.contents.depth, (n,)), np.ctypeslib.as_array(ms.contents.info, (n,))


def host_summary(ms, path):
    with mg.CFile(path, "w") as f:
        mg.lib().modsetSummary(ms, f)
    return open(path).read()


def histogram(ms, path):
    with mg.CFile(path, "w") as f:
        mg.lib().mgDepthHistogram(ms, f)
    return open(path).read()
