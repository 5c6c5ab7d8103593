"""The host parser taken up in the MIDDLE of an ordinary gzip file (mg_seqio.c seqOpenAt through the hook mgSeqOpenAt): the device text
parser reads such a file too (mg_gzipsrc.hip) and hands it over at a TEXT offset -- a FASTQ file that breaks a rule, a FASTA or FASTQ
file that ends unfinished.  A deflate stream has no index, so the reader inflates the text before the offset and drops it.  Against the
plain file opened at the same offset: the same records, ids and line numbers in the messages, for every record start, for one member
and for two (the cut inside a record, so that starts lie in both), FASTA and FASTQ."""
import gzip

import numpy as np
import pytest

from tests.test_gpu_text import crafted_fasta
from tests.test_seqio_bgzf_from import N_REC, fastq_text, records_from, same


def fasta_text():
    """a crafted FASTA text and (offset, line number) of every record's '>'"""
    text = crafted_fasta(np.random.default_rng(41), 30, "mixed")
    starts = [(0, 1)] + [(i + 1, text.count(b"\n", 0, i + 1) + 1) for i in range(len(text) - 1) if text[i:i + 2] == b"\n>"]
    return text, starts


def one_member(text):
    return gzip.compress(text, 6)


def two_members(text):
    cut = len(text) // 2 + 7
    return gzip.compress(text[:cut], 6) + gzip.compress(text[cut:], 1)


@pytest.mark.parametrize("pack", [one_member, two_members])
def test_fastq_every_record_start_as_start_offset(pack, tmp_path, capfd):
    """the file ends in the middle of a 41st record: the message names the FILE's line, wherever the reader was opened"""
    text, starts = fastq_text()
    text += b"@cut short\nACGT\n"
    plain, gz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text); open(gz, "wb").write(pack(text))
    whole = records_from(plain, 0, 1, 0)
    capfd.readouterr()
    for i in range(N_REC):
        want = records_from(plain, starts[i], 4 * i + 1, i)
        err_want = capfd.readouterr().err
        got = records_from(gz, starts[i], 4 * i + 1, i)
        err_got = capfd.readouterr().err
        assert want is not None and got is not None, i
        assert want[0] == whole[0][i:] and same(got, want), i
        assert "incomplete sequence record line %d" % (4 * N_REC + 3) in err_want and err_got == err_want, (i, err_got, err_want)


@pytest.mark.parametrize("pack", [one_member, two_members])
def test_fasta_every_record_start_as_start_offset(pack, tmp_path, capfd):
    """FASTA whose last line has no newline: 'incomplete sequence record line N' with the file's line number"""
    text, starts = fasta_text()
    text = text[:-1]
    assert not text.endswith(b"\n") and len(starts) >= 10
    plain, gz = str(tmp_path / "t.fa"), str(tmp_path / "t.fa.gz")
    open(plain, "wb").write(text); open(gz, "wb").write(pack(text))
    whole = records_from(plain, 0, 1, 0)
    err_whole = capfd.readouterr().err
    assert "incomplete sequence record line" in err_whole
    for i, (off, line) in enumerate(starts):
        want = records_from(plain, off, line, i)
        err_want = capfd.readouterr().err
        got = records_from(gz, off, line, i)
        err_got = capfd.readouterr().err
        if want is None:
            assert got is None, i
            continue
        assert got is not None and want[0] == whole[0][i:] and same(got, want), i
        assert err_want == err_whole and err_got == err_want, (i, err_got, err_want)


def test_small_batches_from_the_second_member(tmp_path):
    text, starts = fastq_text()
    plain, gz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text); open(gz, "wb").write(two_members(text))
    cut = len(text) // 2 + 7
    late = [i for i in range(N_REC) if starts[i] > cut]
    assert late and late[0] > 1
    for i in (late[0], late[-1]):
        assert same(records_from(gz, starts[i], 4 * i + 1, i, 1), records_from(plain, starts[i], 4 * i + 1, i, 1)), i


def test_start_at_or_past_the_end_is_refused(tmp_path):
    text, starts = fastq_text()
    plain, gz = str(tmp_path / "t.fq"), str(tmp_path / "t.fq.gz")
    open(plain, "wb").write(text); open(gz, "wb").write(two_members(text))
    for off in (len(text), len(text) + 1, len(text) + 100000):
        assert records_from(plain, off, 1, 0) is None and records_from(gz, off, 1, 0) is None, off
    assert len(records_from(gz, starts[N_REC - 1], 4 * N_REC - 3, N_REC - 1)[0]) == 1      # the last record start is taken
    assert same(records_from(gz, 0, 1, 0), records_from(plain, 0, 1, 0))
