"""A file's bytes cross to the device in page-locked pieces, one read while the piece before it is on the link (csrc/mg_devfile.h): 16 MiB each, so no
other test's file reaches a second piece, let alone the third, which waits for the first one's copy.  MODGPU_FILE_PIECE_KB=4 cuts files of a few
KiB into pieces: bgzip (mgBgzfDeflateFile, a piece a call), gzip -dc (mgGzipInflateFile, the whole file in one call), and a BGZF file both ways it is
read -- resident for the two walks of mgCompositionFile / mgSeqConvertFile, and through the ring of the text parser's single walk.  Every result is
compared with Python's zlib / gzip or with the same call at the default piece; every case says how many pieces its file spans."""
import gzip
import os
import zlib

import numpy as np
import pytest

import modimizer_amd as mg
from tests.test_gpu_text import device_records

pytestmark = pytest.mark.gpu

PIECE = 4096
ALL_COMP = mg.COMP_BASES | mg.COMP_QUALS | mg.COMP_LENGTHS


def pieces(size):
    return -(-size // PIECE)


def acgt_lines(n, seed):
    """n bytes: pseudo-random ACGT in lines of 60"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    a[60::61] = 10
    return a.tobytes()


def fasta(n, seed):
    """about n bytes of FASTA: records of 50 lines of 60 pseudo-random bases"""
    body = acgt_lines(n, seed).split(b"\n")
    out = []
    for i in range(0, len(body), 50):
        out.append(b">rec%d piece test\n" % (i // 50) + b"\n".join(body[i:i + 50]) + b"\n")
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------- bgzip
@pytest.mark.parametrize("size,spans", [(0, 0), (4095, 1), (4096, 1), (4097, 2), (8192, 2), (12289, 4), (5 * 4096 + 1, 6)])
def test_bgzip_a_piece_a_call(size, spans, tmp_path):
    assert pieces(size) == spans
    text = acgt_lines(size, size)
    src, small, dflt = (str(tmp_path / n) for n in ("in.txt", "small.gz", "default.gz"))
    open(src, "wb").write(text)
    with mg.knobs(FILE_PIECE_KB=4):
        mg.bgzf_deflate_file(src, small)
    mg.bgzf_deflate_file(src, dflt)
    blob = open(small, "rb").read()
    assert gzip.decompress(blob) == text                   # (every member, the empty last one too)
    assert blob == open(dflt, "rb").read()                 # a member is a function of its block alone


# ---------------------------------------------------------------------------------------------------------------- gzip -dc
def gunzip_in_pieces(blob, tmp_path, **knobs):
    src, dst = str(tmp_path / "in.gz"), str(tmp_path / "out.txt")
    open(src, "wb").write(blob)
    with mg.knobs(FILE_PIECE_KB=4, **knobs):
        assert mg.gzip_inflate_file(src, dst)
        d = mg.inflate_diag()
    assert open(dst, "rb").read() == gzip.decompress(blob)
    assert d["uploaded"] == len(blob), d


@pytest.mark.parametrize("size,spans", [(4096, 1), (4097, 2), (8192, 2), (8193, 3), (12288, 3), (12289, 4)])
def test_gunzip_a_stored_member_on_and_past_a_piece_edge(size, spans, tmp_path):
    """level 0: the header's 10 bytes, one stored block (5 bytes and the text), the trailer's 8"""
    text = acgt_lines(size - 23, size)
    blob = gzip.compress(text, 0, mtime=0)
    assert len(blob) == size and pieces(len(blob)) == spans
    gunzip_in_pieces(blob, tmp_path)


def test_gunzip_a_deflated_file_of_more_than_five_pieces(tmp_path):
    blob = gzip.compress(acgt_lines(96 << 10, 7), 6, mtime=0)
    assert len(blob) > 5 * PIECE and pieces(len(blob)) >= 6
    gunzip_in_pieces(blob, tmp_path, GZIP_CHUNK_KB=4)


# ---------------------------------------------------------------------------------------------------------------- BGZF, both routes
_bgzf = {}


def bgzf_file(tmp_path_factory):
    """(path, blob, the plain text): at least five pieces and a part of one, made once"""
    if not _bgzf:
        text = fasta(100 << 10, 11)
        blob = mg.bgzf_bytes(text, block=4096)
        path = str(tmp_path_factory.mktemp("pieces") / "t.fa.gz")
        open(path, "wb").write(blob)
        _bgzf["file"] = (path, blob, text)
    path, blob, text = _bgzf["file"]
    assert pieces(len(blob)) >= 6 and len(blob) % PIECE
    return path, blob, text


def comp_call(path):
    out, err, res = mg.composition_file(path, ALL_COMP)
    return out, err, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in res.items()}


def test_bgzf_resident_for_two_walks(tmp_path, tmp_path_factory):
    path, blob, text = bgzf_file(tmp_path_factory)
    a, b = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
    with mg.knobs(TEXT_WINDOW_KB=4):
        want_comp = comp_call(path)
        want_conv = mg.seq_convert_file(path, a, mg.SEQ_FASTA)
    with mg.knobs(TEXT_WINDOW_KB=4, FILE_PIECE_KB=4):
        assert comp_call(path) == want_comp
        d = mg.inflate_diag()
        assert d["uploaded"] == len(blob) and d["text"] == len(text), d
        assert mg.seq_convert_file(path, b, mg.SEQ_FASTA) == want_conv
        d = mg.inflate_diag()
        assert d["uploaded"] == len(blob) and d["text"] > len(text), d      # two walks inflate, one uploads
    assert open(a, "rb").read() == open(b, "rb").read()
    assert want_comp[2]["totLen"] == sum(len(line) for line in text.split(b"\n") if not line.startswith(b">"))


def test_bgzf_through_the_ring_of_the_text_parser(tmp_path_factory):
    path, blob, text = bgzf_file(tmp_path_factory)
    with mg.knobs(TEXT_WINDOW_KB=4):
        rc, want = device_records(path)
    assert rc == 0, mg.lib().mgLastError()
    with mg.knobs(TEXT_WINDOW_KB=4, FILE_PIECE_KB=4):
        rc, got = device_records(path)
        diag, d = mg.text_file_diag(), mg.inflate_diag()
    assert rc == 0, mg.lib().mgLastError()
    assert diag["path"] == 2 and diag["text"] == len(text)
    assert d["uploaded"] == len(blob), d
    assert len(got) == len(want) == text.count(b">")
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
