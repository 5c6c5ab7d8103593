"""modutils -x on the GPU (modutils.c:33-51 with is10x): mgAddSequenceFile10x, mgAddSequenceBatch10x and mgTrim10xDevice against the
reference program's own files (tests/golden/tenx_*, made by make_golden_tenx.py), against the 10x rule restated in numpy and the CPU
oracle, at every edge of the parser's windows and batches, and through the host parser's legs.  mgAdd10xDiag says which legs ran."""
import ctypes as C
import gzip

import numpy as np
import pytest

import modimizer_amd as mg
import util
import tenx_util as tx

pytestmark = pytest.mark.gpu
INPUTS = ["fq", "fa"]


def input_text(ext):
    return open(tx.gpath("tenx_reads." + ext), "rb").read()


def check_against_golden(ms, tag, ext, added, tmp_path):
    """the added line, the depths (-H), and after -s / -sM the table (-wt), the .mod and every summary, all before anything is synced"""
    L = mg.lib()
    line, (after_x, after_s, after_sm) = tx.golden_lines(tag, ext)
    assert added == line
    assert tx.histogram(ms, str(tmp_path / "his.txt")) == util.golden_text("tenx_%s_%s.hist.txt" % (tag, ext))
    assert mg.summary_device(ms, str(tmp_path / "s0.txt")) == after_x
    assert mg.set_copy(ms, *tx.COPY) == 0
    assert mg.summary_device(ms, str(tmp_path / "s1.txt")) == after_s
    assert mg.set_copy_m(ms, tx.COPY_M) == 0
    assert mg.summary_device(ms, str(tmp_path / "s2.txt")) == after_sm
    mg.write_text_device(ms, str(tmp_path / "dump.txt"))
    assert open(tmp_path / "dump.txt").read() == util.golden_text("tenx_%s_%s.dump.txt" % (tag, ext))
    with mg.CFile(str(tmp_path / "out.mod"), "w") as f:
        L.modsetWrite(ms, f)
    got, want = open(tmp_path / "out.mod", "rb").read(), tx.golden_mod(tag, ext)[0]
    v0 = 24 + C.sizeof(mg.Seqhash) + 4 * (1 << tx.TAGS[tag][0])      # value[0] is no entry: modsetCreate leaves it as malloc gave it
    assert got[:v0] == want[:v0] and got[v0 + 8:] == want[v0 + 8:]
    assert tx.host_summary(ms, str(tmp_path / "h.txt")) == after_sm


def check_against_oracle(ms, params, batches, hashes=None):
    oms, want_hashes = tx.oracle_set(params, batches)
    mg.check(mg.lib().modsetSyncToHost(ms, 0))
    v, d, _ = mg.modset_arrays(ms)
    assert ms.contents.max == oms.max
    assert np.array_equal(v[1:], oms.values()[1:]) and np.array_equal(d[1:], oms.depths()[1:])
    if hashes is not None:
        assert list(hashes) == want_hashes
    return oms


# ---- 1: the file entry against the reference ----------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", INPUTS)
@pytest.mark.parametrize("tag", list(tx.TAGS))
def test_file_10x_matches_reference(tag, ext, tmp_path):
    ms = tx.new_set(tag)
    n = len(tx.file_reads(input_text(ext)))
    diag = mg.add_sequence_file_10x(ms, tx.gpath("tenx_reads." + ext), str(tmp_path / "added.txt"))
    assert diag == (1, (n + 1) // 2, tx.SKIP * ((n + 1) // 2), 0)      # one batch, trimmed on the device; no leg of the host parser
    check_against_golden(ms, tag, ext, open(tmp_path / "added.txt").read(), tmp_path)
    tx.destroy(ms)


@pytest.mark.parametrize("ext", INPUTS)
def test_windows_and_batches_cut_after_odd_and_even_records(ext, tmp_path):
    """windows of 4 KiB, a batch handed on at every window's end: the records handed on before a batch say which of its records are the
    odd ones, whether that count is odd or even"""
    tag = "k11w4"
    text = input_text(ext)
    cuts = [text[:e] for e in range(4096, len(text), 4096)]
    edges = [p.count(b"\n") // 4 if ext == "fq" else p.count(b"\n>") for p in cuts]
    assert len(edges) >= 2 and {e % 2 for e in edges} == {0, 1}, edges
    n = len(tx.file_reads(text))
    ms = tx.new_set(tag)
    with mg.knobs(TEXT_WINDOW_KB=4, FILE_BATCH_BASES=100):
        diag = mg.add_sequence_file_10x(ms, tx.gpath("tenx_reads." + ext), str(tmp_path / "added.txt"))
    assert diag == (len(edges) + 1, (n + 1) // 2, tx.SKIP * ((n + 1) // 2), 0)
    check_against_golden(ms, tag, ext, open(tmp_path / "added.txt").read(), tmp_path)
    tx.destroy(ms)


# ---- 2: the host parser's legs ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["gzip", "no_final_newline"])
@pytest.mark.parametrize("ext", INPUTS)
def test_host_parser_legs(ext, how, tmp_path, capfd):
    """the golden files gzip'd: the reference's own result.  Without the final newline the last record is incomplete: the readers report
    it and do not deliver it (seqio.c:213-217), so the result is the oracle's on the records before it"""
    tag = "k25w3"
    text = input_text(ext)
    reads = tx.file_reads(text)
    if how == "gzip":
        path = str(tmp_path / ("reads.%s.gz" % ext))
        with gzip.open(path, "wb") as f:
            f.write(text)
    else:
        path = str(tmp_path / ("reads." + ext))
        open(path, "wb").write(text[:-1])
        reads = reads[:-1]
    n = len(reads)
    ms = tx.new_set(tag)
    diag = mg.add_sequence_file_10x(ms, path, str(tmp_path / "added.txt"))
    assert diag == (1, (n + 1) // 2, tx.SKIP * ((n + 1) // 2), 1)
    added = open(tmp_path / "added.txt").read()
    if how == "gzip":
        check_against_golden(ms, tag, ext, added, tmp_path)
    else:
        assert "incomplete sequence record" in capfd.readouterr().err
        oms, hashes = tx.oracle_set(tag, [tx.trim(reads)])
        assert added == "added %d sequences total length %d total hashes %d, new max %d\n" % (n, sum(len(r) for r in reads), hashes[0], oms.max)
        check_against_oracle(ms, tag, [tx.trim(reads)])
    tx.destroy(ms)


@pytest.mark.parametrize("keep", [60, 85])
def test_fastq_hand_over_in_the_middle(keep, tmp_path, capfd):
    """the file ends inside record keep + 1: the device parser hands on the records of its whole windows, the host parser takes the
    rest from the first record not yet added (the -3 hand-over) and goes on numbering where the device stopped -- after an odd count
    (keep = 60: the 51 records of two windows of 4 KiB) and after an even one (keep = 85: the 68 of three)"""
    tag = "k11w4"
    lines = input_text("fq").split(b"\n")
    text = b"\n".join(lines[:4 * keep + 2]) + b"\n"            # keep records, then a header and a sequence line
    path = str(tmp_path / "cut.fq")
    open(path, "wb").write(text)
    handed = text[:(len(text) - 1) // 4096 * 4096].count(b"\n") // 4
    assert 0 < handed < keep and handed == (51 if keep == 60 else 68), handed
    reads = tx.file_reads(text)[:keep]
    ms = tx.new_set(tag)
    with mg.knobs(TEXT_WINDOW_KB=4, FILE_BATCH_BASES=100):
        diag = mg.add_sequence_file_10x(ms, path, str(tmp_path / "added.txt"))
    assert "incomplete sequence record" in capfd.readouterr().err
    assert diag[0] >= 3 and diag[1:] == ((keep + 1) // 2, sum(min(tx.SKIP, len(r)) for r in reads[0::2]), 1)
    oms = check_against_oracle(ms, tag, [tx.trim(reads)])
    total, hashes = sum(len(r) for r in reads), tx.oracle_set(tag, [tx.trim(reads)])[1][0]
    assert open(tmp_path / "added.txt").read() == "added %d sequences total length %d total hashes %d, new max %d\n" % (keep, total, hashes, oms.max)
    tx.destroy(ms)


# ---- 3: the trim alone ---------------------------------------------------------------------------------------------------------

def unpack(words, n):
    w = np.repeat(words[:(n + 15) // 16], 16)[:n]
    return ((w >> (30 - 2 * (np.arange(n) % 16)).astype(np.uint32)) & 3).astype(np.uint8)


@pytest.fixture(scope="module")
def trim_batch():
    """about 300 records: every length at which the trim or the gather's words change hands, runs of empty records, and random ones up
    to 200 bases, so that an output word spans several records and several empty ones"""
    rng = np.random.default_rng(23)
    fixed = [0, 1, 15, 16, 17, 22, 23, 24, 39, 40]
    lens = fixed + [0, 0, 0, 23, 0, 22, 1, 23, 23, 0, 5, 23, 3, 0, 0, 24, 2] + [int(x) for x in rng.integers(0, 201, 270)] + fixed[::-1]
    reads = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    return reads


@pytest.mark.parametrize("first", [1, 2])
def test_trim_device_against_numpy(trim_batch, first):
    L = mg.lib()
    reads = trim_batch
    bases, offs = util.concat_reads(reads)
    total, n = int(offs[-1]), len(reads)
    want = tx.trim(reads, first)
    wb, wo = util.concat_reads(want)
    assert int(wo[-1]) == total - sum(min(tx.SKIP, len(r)) for i, r in enumerate(reads) if (first + i) & 1)
    d_in = mg.DeviceBuffer.from_numpy(mg.pack_host(bases))
    d_off = mg.DeviceBuffer.from_numpy(offs.astype(np.uint64))
    nw = L.mgPackedWords(total)
    d_out = mg.DeviceBuffer.from_numpy(np.full(nw, 0xffffffff, np.uint32))      # every word of the result is written, the pad too
    d_oo = mg.DeviceBuffer((n + 1) * 8)
    tot = C.c_uint64()
    mg.check(L.mgTrim10xDevice(d_in.ptr, total, d_off.ptr, n, first, d_out.ptr, d_oo.ptr, C.byref(tot), None))
    assert tot.value == int(wo[-1])
    assert np.array_equal(d_oo.to_numpy(np.uint64, n + 1), wo.astype(np.uint64))
    got = d_out.to_numpy(np.uint32, nw)
    nwo = L.mgPackedWords(tot.value)
    assert np.array_equal(got[:nwo], mg.pack_host(wb)) and np.all(got[nwo:] == 0xffffffff)
    assert np.array_equal(unpack(got, tot.value), wb)
    for b in (d_in, d_off, d_out, d_oo):
        b.free()


def test_trim_device_edges():
    """no records; records that are all barcode (the result holds no base); more records than the 32-bit sum of the skips allows"""
    L = mg.lib()
    tot = C.c_uint64(99)
    d_off = mg.DeviceBuffer.from_numpy(np.zeros(1, np.uint64)); d_p = mg.DeviceBuffer(L.mgPackedWords(0) * 4 + 64); d_oo = mg.DeviceBuffer(64)
    mg.check(L.mgTrim10xDevice(d_p.ptr, 0, d_off.ptr, 0, 1, d_p.ptr, d_oo.ptr, C.byref(tot), None))
    assert tot.value == 0 and d_oo.to_numpy(np.uint64, 1)[0] == 0
    reads = [np.ones(n, np.uint8) for n in (23, 0, 7, 0, 23)]
    bases, offs = util.concat_reads(reads)
    d_in = mg.DeviceBuffer.from_numpy(mg.pack_host(bases)); d_o2 = mg.DeviceBuffer.from_numpy(offs.astype(np.uint64))
    d_out = mg.DeviceBuffer(L.mgPackedWords(len(bases)) * 4); d_oo2 = mg.DeviceBuffer(6 * 8)
    mg.check(L.mgTrim10xDevice(d_in.ptr, len(bases), d_o2.ptr, 5, 1, d_out.ptr, d_oo2.ptr, C.byref(tot), None))
    assert tot.value == 0 and not d_oo2.to_numpy(np.uint64, 6).any()
    assert not d_out.to_numpy(np.uint32, L.mgPackedWords(0)).any()
    assert L.mgTrim10xDevice(d_in.ptr, len(bases), d_o2.ptr, 0xffffffff // 23 + 1, 1, d_out.ptr, d_oo2.ptr, C.byref(tot), None) != 0
    assert b"32 bits" in L.mgLastError()
    for b in (d_off, d_p, d_oo, d_in, d_o2, d_out, d_oo2):
        b.free()


# ---- 4: with what the set holds already -------------------------------------------------------------------------------------------

def test_x_after_a_on_one_set_and_x_is_not_a(tmp_path):
    """-a, a sync (base depths), -a again and -x (pending depths on top of them), with a record shorter than 23 bases at an odd place
    in a batch of its own: an empty read, the library's rule.  And -x alone is not -a: the barcodes of k <= 23 would have hashed."""
    L = mg.lib()
    tag = "k11w4"
    fq, fa = tx.file_reads(input_text("fq")), tx.file_reads(input_text("fa"))
    ms = tx.new_set(tag)
    with mg.CFile(str(tmp_path / "a.txt"), "w") as f:
        assert L.mgAddSequenceFile(ms, tx.gpath("tenx_reads.fa").encode(), f) == 0
    mg.check(L.modsetSyncToHost(ms, 0))
    with mg.CFile(str(tmp_path / "a.txt"), "a") as f:
        assert L.mgAddSequenceFile(ms, tx.gpath("tenx_reads.fq").encode(), f) == 0
    diag = mg.add_sequence_file_10x(ms, tx.gpath("tenx_reads.fq"), str(tmp_path / "a.txt"), "a")
    assert diag[0] == 1 and diag[3] == 0
    short = [fq[20][:9], fq[21], fq[22][:22], fq[23], fq[24]]   # records 1 and 3 are shorter than the barcode
    bases, offs = util.concat_reads(short)
    h = L.mgAddSequenceBatch10x(ms, bases.ctypes.data, offs.ctypes.data, len(short), 1)
    assert [len(r) for r in tx.trim(short)[0:3:2]] == [0, 0]
    batches = [fa, fq, tx.trim(fq), tx.trim(short)]
    oms, hashes = tx.oracle_set(tag, batches)
    assert h == hashes[3] > 0
    lines = open(tmp_path / "a.txt").read().splitlines()
    assert [int(l.split()[8].rstrip(",")) for l in lines] == hashes[:3] and hashes[1] != hashes[2]
    # pending counts on top of synced ones: the summary counted on the device is the oracle's set's
    dev = mg.summary_device(ms, str(tmp_path / "d.txt"))
    check_against_oracle(ms, tag, batches)
    assert dev == tx.host_summary(ms, str(tmp_path / "h.txt"))
    tx.destroy(ms)
    # the same file through -a and through -x: other sets
    a, x = tx.oracle_set(tag, [fq])[0], tx.oracle_set(tag, [tx.trim(fq)])[0]
    assert a.max != x.max
