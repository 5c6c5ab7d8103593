"""The host parser taken up in the MIDDLE of a blocked-gzip (BGZF) file (mg_seqio.c seqOpenAt through the hook mgSeqOpenAt): where the
device text parser hands a FASTQ file over (mg_textgpu.hip, -3) it names a TEXT offset, and for BGZF the reader walks the members'
headers to the one that holds it and drops the bytes before it.  Against the plain file opened at the same offset: the same records,
ids, record count and line numbers in the messages, for every record start of a 40-record file and members of 64, 1000 and 65280
bytes -- so that a start falls inside, at the first byte of and at the last byte of a member."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests.test_gpu_text import crafted_fastq

N_REC = 40
BLOCKS = [64, 1000, 65280]


def fastq_text():
    """40 crafted records (the first of exactly 64 bytes, so that record 1 starts at the first byte of a 64-byte member and record 0's
    last newline is a member's last byte) and the start offset of every one of them"""
    text = crafted_fastq(np.random.default_rng(40), N_REC)
    lines = text.split(b"\n")[:-1]
    recs = [b"\n".join(lines[4 * i:4 * i + 4]) + b"\n" for i in range(N_REC)]
    recs[0] = b"@first id\n" + b"ACGTN" * 5 + b"\n+\n" + b"I" * 25 + b"\n"
    recs[1] = b"@secon\n" + b"C" * 26 + b"\n+\n" + b"F" * 26 + b"\n"
    assert len(recs[0]) == 64 and len(recs[1]) == 63        # ... and record 2 at the last byte of one
    starts = list(np.cumsum([0] + [len(r) for r in recs]))
    return b"".join(recs), [int(s) for s in starts]


def records_from(path, off, line, seq, max_bases=1 << 40):
    """every record the reader opened at (off, line, seq) returns: (ids, bases), or None if it does not open"""
    L = mg.lib()
    r = L.mgSeqOpenAt(path.encode(), off, line, seq)
    if not r:
        return None
    names, seqs = [], []
    b = mg.MgSeqBatch()
    while True:
        n = L.mgSeqNextBatch(r, max_bases, C.byref(b))
        if n == 0:
            break
        offs = np.ctypeslib.as_array(b.offsets, shape=(n + 1,)).copy()
        bases = np.ctypeslib.as_array(b.bases, shape=(max(int(b.total), 1),))[:b.total].astype(np.uint8)
        for i in range(n):
            names.append(b.names[i].decode()); seqs.append(bases[offs[i]:offs[i + 1]].copy())
        L.mgSeqBatchFree(C.byref(b))
    L.mgSeqClose(r)
    return names, seqs


def same(a, b):
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_hook_is_exported():
    assert "mgSeqOpenAt" in mg.EXPORTS and hasattr(mg.lib(), "mgSeqOpenAt")


@pytest.mark.parametrize("block", BLOCKS)
def test_every_record_start_as_start_offset(block, tmp_path, capfd):
    """the file ends in the middle of a 41st record, after two of its lines: the reader says so with the FILE's line number -- the line the
    text runs out at, 4 * 40 + 3 (seqio.c:213-217) -- wherever it was opened"""
    text, starts = fastq_text()
    text += b"@cut short\nACGT\n"
    plain, bgz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text)
    blob = mg.bgzf_bytes(text, block=block)
    open(bgz, "wb").write(blob)
    members = mg.bgzf_members(blob)
    firsts = {m[2] for m in members if m[3]}; lasts = {m[2] + m[3] - 1 for m in members if m[3]}
    if block == 64:                                         # the three places a start can take in a member all occur
        assert any(s in firsts for s in starts[1:N_REC]) and any(s in lasts for s in starts[1:N_REC])
        assert any(s not in firsts and s not in lasts for s in starts[1:N_REC])
    whole = records_from(plain, 0, 1, 0)
    assert len(whole[0]) == N_REC
    capfd.readouterr()
    for i in range(N_REC):
        want = records_from(plain, starts[i], 4 * i + 1, i)
        err_want = capfd.readouterr().err
        got = records_from(bgz, starts[i], 4 * i + 1, i)
        err_got = capfd.readouterr().err
        assert want is not None and got is not None, i
        assert len(want[0]) == N_REC - i and want[0] == whole[0][i:]
        assert same(got, want), i
        assert "incomplete sequence record line %d" % (4 * N_REC + 3) in err_want and err_got == err_want, (i, err_got, err_want)


@pytest.mark.parametrize("block", BLOCKS)
def test_small_batches_from_the_middle(block, tmp_path):
    """batches of one record: the reader refills across members after the bytes in front were dropped"""
    text, starts = fastq_text()
    plain, bgz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text); open(bgz, "wb").write(mg.bgzf_bytes(text, block=block))
    for i in (1, 17, N_REC - 1):
        assert same(records_from(bgz, starts[i], 4 * i + 1, i, 1), records_from(plain, starts[i], 4 * i + 1, i, 1)), i


@pytest.mark.parametrize("block", BLOCKS)
def test_fatal_message_carries_the_files_line(block, tmp_path):
    """a record without its '+' behind the start offset: the reader dies with the reference's message and the FILE's line number, as it
    does on the plain file opened at the same offset"""
    text, starts = fastq_text()
    bad = 33
    lines = text.split(b"\n")
    assert lines[4 * bad + 2].startswith(b"+")
    lines[4 * bad + 2] = b"-" + lines[4 * bad + 2][1:]
    text = b"\n".join(lines)
    plain, bgz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text); open(bgz, "wb").write(mg.bgzf_bytes(text, block=block))
    i = 20
    code = ("import ctypes as C, modimizer_amd as mg; L = mg.lib(); r = L.mgSeqOpenAt(%r.encode(), %d, %d, %d); assert r; b = mg.MgSeqBatch()\n"
            "while L.mgSeqNextBatch(r, 1 << 40, C.byref(b)): print(b.nSeq, flush=True)")
    res = []
    for path in (plain, bgz):
        r = subprocess.run([sys.executable, "-c", code % (path, starts[i], 4 * i + 1, i)], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=util.ROOT))
        res.append((r.returncode, r.stdout, r.stderr))
    assert res[0] == res[1], res
    assert res[0][0] != 0 and "missing + FASTQ line %d" % (4 * bad + 3) in res[0][2], res[0]


def test_start_at_or_past_the_end_is_refused(tmp_path):
    text, starts = fastq_text()
    plain, bgz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text); open(bgz, "wb").write(mg.bgzf_bytes(text, block=1000))
    for off in (len(text), len(text) + 1, len(text) + 100000):
        assert records_from(plain, off, 1, 0) is None and records_from(bgz, off, 1, 0) is None, off
    assert len(records_from(bgz, starts[N_REC - 1], 4 * N_REC - 3, N_REC - 1)[0]) == 1      # the last record start is taken


def test_empty_member_in_the_middle(tmp_path):
    """two bgzip files concatenated: the first one's end-of-file marker, an empty member, lies in mid-file -- before, at and after the
    start offset"""
    text, starts = fastq_text()
    half = starts[N_REC // 2]
    plain, bgz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text)
    blob = mg.bgzf_bytes(text[:half], block=300, eof=True) + mg.bgzf_bytes(text[half:], block=300, eof=True)
    open(bgz, "wb").write(blob)
    assert sum(1 for m in mg.bgzf_members(blob) if m[3] == 0) == 2
    for i in (0, 3, N_REC // 2 - 1, N_REC // 2, N_REC // 2 + 1, N_REC - 1):
        got, want = records_from(bgz, starts[i], 4 * i + 1, i), records_from(plain, starts[i], 4 * i + 1, i)
        assert got is not None and same(got, want) and len(got[0]) == N_REC - i, i
