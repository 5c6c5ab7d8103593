"""Ordinary gzip inflated on the device (csrc/mg_gunzip.hip, mg_gzipsrc.hip): the corpus of tests/test_gunzip_host.py through mgGzipInflateFile against
the host compile of the same pipeline -- bytes and all eight counters of mgGunzipDiag -- then mgCompositionFile and mgSeqConvertFile on gzip files
against the plain files, the knobs, an unfinished record, a corrupt stream, and the file that keeps the host path."""
import gzip
import os

import pytest

import modimizer_amd as mg
from tests import test_composition as tc
from tests import test_gunzip_host as th

pytestmark = pytest.mark.gpu

ALL_COMP = mg.COMP_BASES | mg.COMP_QUALS | mg.COMP_LENGTHS
WINDOWS = [None, 4]
CHUNK_KB = [4, 32]
ZERO = dict.fromkeys(mg.GUNZIP_DIAG, 0)
# of th.KNOBS (chunk bytes, chunks a batch, capacity guess): every chunk size, both batch sizes, both guesses, in four runs a file
KNOBS = [(4096, 3, 1), (4096, 64, 64), (16384, 64, 1), (32768, 3, 64)]


def device_inflate(m, chunk, batch, ratio, tmp_path):
    """(text or None, error message, mgGunzipDiag) of mgGzipInflateFile at these knobs"""
    src, dst = str(tmp_path / "in.gz"), str(tmp_path / "out.txt")
    open(src, "wb").write(m["blob"])
    if os.path.exists(dst):
        os.remove(dst)
    with mg.knobs(GZIP_CHUNK_KB=chunk // 1024, GZIP_BATCH=batch, GZIP_RATIO=ratio):
        try:
            took = mg.gzip_inflate_file(src, dst)
        except mg.ModgpuError as e:
            assert not os.path.exists(dst), "a failed call left an output file"
            return None, str(e), mg.gunzip_diag()
        d = mg.gunzip_diag()
    if not took:
        assert not os.path.exists(dst)
        return None, "not gzip", d
    return open(dst, "rb").read(), "", d


@pytest.mark.parametrize("m", th.good_corpus(), ids=lambda m: m["name"])
def test_good_file_equals_the_host_compile(m, tmp_path):
    for chunk, batch, ratio in KNOBS:
        status, want, hd, _ = mg.gunzip_host(m["blob"], chunk, batch, chunk * ratio, len(m["text"]))
        assert status == 0 and want == m["text"]
        text, err, d = device_inflate(m, chunk, batch, ratio, tmp_path)
        assert text == want, (m["name"], chunk, batch, ratio, err)
        assert d == hd, (m["name"], chunk, batch, ratio)


def corrupt_against_host(ms, tmp_path, knobs=((4096, 3, 1), (16384, 64, 64))):
    for i, m in enumerate(ms):
        for chunk, batch, ratio in knobs[i % 2:i % 2 + 1]:   # (the two runs take turns: the host test crosses every file with every knob)
            status, want, hd, _ = mg.gunzip_host(m["blob"], chunk, batch, chunk * ratio, 1 << 23)      # (room that never binds: the device's does not)
            text, err, d = device_inflate(m, chunk, batch, ratio, tmp_path)
            what = (m["name"], chunk, batch, ratio, err)
            if status:
                assert text is None, what
                if err != "not gzip":                       # (what is no gzip header at the file's start is declined, not inflated)
                    assert "offset" in err and "status %d)" % status in err, what
            else:
                assert text == want == th.zlib_verdict(m["blob"]), what
            if err != "not gzip":
                assert d == hd, what


def test_corrupt_files_get_the_hosts_verdict(tmp_path):
    corrupt_against_host(th.corrupt_corpus()[:-70], tmp_path)


def test_cut_files_get_the_hosts_verdict(tmp_path):
    corrupt_against_host(th.corrupt_corpus()[-70:-50], tmp_path)


def test_flipped_bits_get_the_hosts_verdict(tmp_path):
    corrupt_against_host(th.corrupt_corpus()[-50:], tmp_path)


# ---------------------------------------------------------------------------------------------------------------- the two calls
def comp_call(path, flags=ALL_COMP):
    out, err, res = mg.composition_file(path, flags)
    return out, err, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in res.items()}


def ran_on_device(d):
    return d["batches"] >= 1 and d["members"] >= 1 and d["confirmed"] >= 1 and d["launches"] == 4 * d["batches"]


@pytest.mark.parametrize("ck", CHUNK_KB)
@pytest.mark.parametrize("kb", WINDOWS)
@pytest.mark.parametrize("name", ["comp_long.fa", "comp_many.fq"])
def test_composition_and_seqconvert_of_a_gzip_file(name, kb, ck, tmp_path):
    plain = os.path.join(tc.GOLDEN, name)
    raw = open(plain, "rb").read()
    path = str(tmp_path / (name + ".gz"))
    open(path, "wb").write(gzip.compress(raw))
    kind = mg.SEQ_FASTA if name.endswith(".fa") else mg.SEQ_FASTQ
    a, b, c = (str(tmp_path / x) for x in ("a.out", "b.out", "c.out"))
    with mg.knobs(TEXT_WINDOW_KB=kb, GZIP_MIN_KB=0, GZIP_CHUNK_KB=ck):
        want = comp_call(plain)
        got = comp_call(path)
        d = mg.gunzip_diag()
        assert got == want
        assert ran_on_device(d) and d["discarded"] == 0, d
        assert mg.inflate_diag()["uploaded"] == os.path.getsize(path) and mg.inflate_diag()["members"] == 0
        assert mg.seq_convert_file(plain, a, kind) == mg.seq_convert_file(path, b, kind)
        d = mg.gunzip_diag()
        assert ran_on_device(d), d                            # (its walks share one upload)
        assert mg.inflate_diag()["uploaded"] == os.path.getsize(path)
        assert open(a, "rb").read() == open(b, "rb").read()
    with mg.knobs(TEXT_WINDOW_KB=kb, GZIP_MIN_KB=0, GZIP_CHUNK_KB=ck, GZIP_HOST=1):
        assert comp_call(path) == want
        assert mg.gunzip_diag() == ZERO and mg.inflate_diag()["uploaded"] == 0
        assert mg.seq_convert_file(path, c, kind) == mg.seq_convert_file(plain, a, kind)
        assert mg.gunzip_diag() == ZERO
        assert open(c, "rb").read() == open(a, "rb").read()


def test_the_default_minimum_keeps_small_files_on_the_host(tmp_path):
    raw = open(os.path.join(tc.GOLDEN, "comp_many.fq"), "rb").read()
    path = str(tmp_path / "small.fq.gz")
    open(path, "wb").write(gzip.compress(raw))
    assert os.path.getsize(path) < 1024 * 1024
    assert comp_call(path) == comp_call(os.path.join(tc.GOLDEN, "comp_many.fq"))
    assert mg.gunzip_diag() == ZERO


@pytest.mark.parametrize("ck", CHUNK_KB)
@pytest.mark.parametrize("kb", WINDOWS)
def test_an_unfinished_last_record(kb, ck, tmp_path):
    """the record is dropped with the program's message and the text is walked again up to the cut: as on the plain file"""
    raw = open(os.path.join(tc.GOLDEN, "comp_many.fq"), "rb").read()[:-7]
    src, path = str(tmp_path / "cut.fq"), str(tmp_path / "cut.fq.gz")
    open(src, "wb").write(raw)
    open(path, "wb").write(gzip.compress(raw))
    with mg.knobs(TEXT_WINDOW_KB=kb, GZIP_MIN_KB=0, GZIP_CHUNK_KB=ck):
        want = comp_call(src)
        got = comp_call(path)
        d = mg.gunzip_diag()
        assert got == want and "incomplete sequence record" in want[1]
        assert ran_on_device(d) and d["batches"] >= 2, d
        a, b = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
        assert mg.seq_convert_file(src, a, mg.SEQ_FASTA) == mg.seq_convert_file(path, b, mg.SEQ_FASTA)
        assert open(a, "rb").read() == open(b, "rb").read()


def test_a_corrupt_stream_fails_the_call(tmp_path):
    raw = open(os.path.join(tc.GOLDEN, "comp_many.fq"), "rb").read()
    blob = bytearray(gzip.compress(raw))
    blob[len(blob) // 2] ^= 0x04
    assert th.zlib_verdict(blob) is None
    path = str(tmp_path / "flipped.fq.gz")
    open(path, "wb").write(blob)
    for kb in WINDOWS:
        with mg.knobs(TEXT_WINDOW_KB=kb, GZIP_MIN_KB=0, GZIP_CHUNK_KB=4):
            with pytest.raises(mg.ModgpuError) as e:
                mg.composition_file(path, ALL_COMP)
            assert path in str(e.value) and "corrupt gzip stream at file offset " in str(e.value), str(e.value)
            assert e.value.out == b""
            dst = str(tmp_path / "o.fq")
            with pytest.raises(mg.ModgpuError) as e:
                mg.seq_convert_file(path, dst, mg.SEQ_FASTQ)
            assert path in str(e.value) and "corrupt gzip stream at file offset " in str(e.value), str(e.value)
            assert not os.path.exists(dst) or os.path.getsize(dst) == 0


def test_a_bc_first_member_keeps_the_host_path(tmp_path):
    """a first member with a 'BC' field in a file that is not BGZF throughout: neither device path is asked"""
    name = "comp_many.fq"
    raw = open(os.path.join(tc.GOLDEN, name), "rb").read()
    half = len(raw) // 2
    path = str(tmp_path / "mixed.gz")
    open(path, "wb").write(mg.bgzf_bytes(raw[:half], 999, eof=False) + gzip.compress(raw[half:]))
    with mg.knobs(GZIP_MIN_KB=0):
        assert comp_call(path) == comp_call(os.path.join(tc.GOLDEN, name))
        assert mg.gunzip_diag() == ZERO and mg.inflate_diag()["members"] == 0
        assert mg.gzip_inflate_file(path, str(tmp_path / "x")) is False and not os.path.exists(str(tmp_path / "x"))
