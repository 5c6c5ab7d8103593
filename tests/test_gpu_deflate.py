"""BGZF deflated on the device (mg_deflate.hip, mg_bgzfsink.hip): the kernel must write, byte for byte, what the encoder's host compile writes
(tests/test_deflate_host.py holds that against zlib); the files of mgBgzfDeflateFile and mgSeqConvertFileBgzf must be the block-by-block
encoding of the whole output text, whatever the window and however the producers cut their appends, and must decompress to what the plain
call writes."""
import functools
import gzip
import os

import numpy as np
import pytest

import modimizer_amd as mg
from tests import test_deflate_host as th
from tests import test_seqconvert as ts

pytestmark = pytest.mark.gpu

MG_ERR_ARG = 3
BLOCKS = [65280, 999, 37]                # MODGPU_BGZF_BLOCK: bgzip's; a few blocks a golden; a block shorter than a line
WINDOWS = [None, 4]                      # MODGPU_TEXT_WINDOW_KB: the parser's default; one tile a window


def host_members(text, block):
    return [mg.deflate_block_host(text[i:i + block])[0] for i in range(0, len(text), block)]


def host_file(text, block):
    return b"".join(host_members(text, block)) + mg.BGZF_EOF


def inflate_on_device(packed, text_bytes):
    members = mg.bgzf_members(packed)
    out, status, bad = mg.inflate_members_device(packed, members, text_bytes)
    assert bad == 0 and not status.any()
    return out.tobytes(), members


# ---- the kernel ----

def test_corpus_in_one_launch_is_the_host_compiles_bytes():
    """every corpus block in one launch: ranges at odd offsets, the first at byte 0, the last ending at the buffer's last byte"""
    want = [(b, m) for name in th.ALL_NAMES for b, m, _, _ in th.encoded(name)]
    buf, ranges = bytearray(), []
    for i, (b, _) in enumerate(want):
        if i:
            buf += b"\x5a" * (1 + 2 * (i % 7))               # an odd gap: the next range starts at an odd or even address in turn
        ranges.append((len(buf), len(b)))
        buf += b
    assert ranges[0][0] == 0 and ranges[-1][0] + ranges[-1][1] == len(buf) and any(off & 1 for off, _ in ranges) and any(off % 8 == 3 for off, _ in ranges)
    packed, off, intact = mg.deflate_blocks_device(bytes(buf), ranges)
    assert intact, "bytes behind memberOff[n] were written"
    run = 0
    for i, (b, m) in enumerate(want):
        assert off[i] == run and packed[off[i]:off[i + 1]] == m, (i, len(b), len(m), off[i + 1] - off[i])
        run += len(m)
    assert off[-1] == run == len(packed)
    d = mg.deflate_diag()
    assert d == dict(blocks=len(want), text=sum(len(b) for b, _ in want), file=run, launches=1)
    # what the device wrote, the device reads: straight into mgInflateMembersDevice
    text, members = inflate_on_device(packed, d["text"])
    assert text == b"".join(b for b, _ in want) and len(members) == len(want)


@functools.lru_cache(maxsize=None)
def small_blocks():
    """1025 blocks of 1 .. 400 bytes cut from the FASTQ text, and their members by the host compile"""
    text = th.long_corpus()[0][1]
    rng = np.random.RandomState(9)
    lens = rng.randint(1, 401, 1025)
    offs = rng.randint(0, len(text) - 400, 1025)
    ranges = [(int(o), int(n)) for o, n in zip(offs, lens)]
    return text, ranges, [mg.deflate_block_host(text[o:o + n])[0] for o, n in ranges]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_launches_of_small_blocks(n):
    text, ranges, want = small_blocks()
    packed, off, intact = mg.deflate_blocks_device(text, ranges[:n])
    assert intact and len(off) == n + 1 and off[0] == 0
    assert [packed[off[i]:off[i + 1]] for i in range(n)] == want[:n]
    assert mg.deflate_diag()["launches"] == 1 and mg.deflate_diag()["blocks"] == n
    back, _ = inflate_on_device(packed, sum(ln for _, ln in ranges[:n]))
    assert back == b"".join(text[o:o + ln] for o, ln in ranges[:n])


def test_refusals_come_before_any_launch():
    text = th.long_corpus()[0][1][:70000]
    for ranges, out_bytes, words in (([(0, 65281)], None, "65280"), ([(0, 100), (69990, 11)], None, "leaves"), ([(1 << 40, 1)], None, "leaves"),
                                     ([(0, 10), (10, 10)], 2 * 65536 - 1, "65536")):
        with pytest.raises(mg.ModgpuError, match=words) as e:
            mg.deflate_blocks_device(text, ranges, out_bytes)
        assert e.value.status == MG_ERR_ARG
        assert mg.deflate_diag() == dict(blocks=0, text=0, file=0, launches=0)
    packed, off, intact = mg.deflate_blocks_device(text, [(0, 10), (10, 10)], 2 * 65536)      # ... and exactly enough is enough
    assert intact and len(packed) == off[2]
    assert mg.deflate_blocks_device(text, []) == (b"", [0], True)


# ---- the files ----

@pytest.mark.parametrize("kb", WINDOWS)
@pytest.mark.parametrize("block", BLOCKS)
def test_bgzf_deflate_file(block, kb, tmp_path):
    src = os.path.join(ts.GOLDEN, "conv_many.fq")
    data = open(src, "rb").read()
    dst, back = str(tmp_path / "many.fq.gz"), str(tmp_path / "many.fq")
    with mg.knobs(BGZF_BLOCK=block, TEXT_WINDOW_KB=kb):
        mg.bgzf_deflate_file(src, dst)
        d = mg.deflate_diag()
        got = open(dst, "rb").read()
        assert got == host_file(data, block), (len(got), len(host_file(data, block)))
        assert d["blocks"] == -(-len(data) // block) and d["text"] == len(data) and d["file"] == len(got) - 28
        assert gzip.decompress(got) == data
        assert mg.bgzf_inflate_file(dst, back) is True and open(back, "rb").read() == data and mg.inflate_diag()["members"] > 0
        empty = tmp_path / "empty"
        empty.write_bytes(b"")
        mg.bgzf_deflate_file(str(empty), dst)
        assert open(dst, "rb").read() == mg.BGZF_EOF and len(mg.BGZF_EOF) == 28
    with pytest.raises(mg.ModgpuError, match="failed to open"):
        mg.bgzf_deflate_file(str(tmp_path / "missing"), dst)
    with pytest.raises(mg.ModgpuError, match="failed to open output"):
        mg.bgzf_deflate_file(src, str(tmp_path / "no" / "such" / "dir.gz"))


def composition(path):
    """(records, bases), or the refusal's words"""
    try:
        c = mg.composition_file(path)[2]
        return c["nSeq"], c["totLen"]
    except mg.ModgpuError as e:
        return str(e)


def converted(stem, path, runs):
    """[(mode, flags)] of a golden that the reference programs convert (test_gpu_seqconvert.py's test_goldens takes the same)"""
    return [(mode, ts.MODES[mode]) for mode, run in runs.items() if ts.expected_of(stem, mode, run)[0] is not None]


@pytest.mark.parametrize("block", BLOCKS)
def test_seqconvert_to_bgzf_is_the_plain_files_text(block, tmp_path):
    """every conv_* golden as FASTA, FASTQ and HOCO: the file is the host compile's members of the plain call's output, cut at `block`, at both window
    sizes -- so the same bytes at both -- with the same counters and stderr; and the device reads it back"""
    crossed = 0
    for stem, path, runs in ts.goldens():
        for mode, flags in converted(stem, path, runs):
            files = []
            for kb in WINDOWS:
                plain, dst = str(tmp_path / "plain"), str(tmp_path / ("out.%s.gz" % ("fq" if mode == "fq" else "fa")))
                with mg.knobs(BGZF_BLOCK=block, TEXT_WINDOW_KB=kb):
                    err0, res0 = mg.seq_convert_file(path, plain, flags)
                    err1, res1 = mg.seqconvert_file_bgzf(path, dst, flags)
                    d = mg.deflate_diag()
                    text, got = open(plain, "rb").read(), open(dst, "rb").read()
                    assert (err1, res1) == (err0, res0), (stem, mode, kb)
                    assert gzip.decompress(got) == text, (stem, mode, kb)
                    assert got == host_file(text, block), (stem, mode, kb)
                    assert d["text"] == len(text) and d["blocks"] == -(-len(text) // block), (stem, mode, kb, d)
                    if text:                                # the project's block-parallel reader takes it: composition on the device path
                        want = composition(plain)
                        assert composition(dst) == want and mg.inflate_diag()["members"] > 0, (stem, mode, kb)
                        assert want[0] == res0["nSeq"] or isinstance(want, str), (stem, mode, kb)
                    if kb and mode == "fq" and path.endswith(".fa") and b"!" * 4097 in text:
                        crossed += 1                        # a '!' run longer than a window: spliced in by hipMemset, in pieces
                files.append(got)
            assert files[0] == files[1], (stem, mode)
    assert crossed >= 1


@pytest.mark.parametrize("kb", WINDOWS)
def test_refusals_are_the_plain_calls(kb, tmp_path):
    src = os.path.join(ts.GOLDEN, "conv_mixed.fa")
    cases = [(path, "out.fa.gz", ts.MODES[mode], True) for stem, path, runs in ts.goldens() if stem.startswith("conv_die_") for mode in runs]
    assert len(cases) >= 6
    # (what is refused before the text is looked at leaves an earlier file alone, in both calls: none is made here)
    cases += [(src, "out.fa.gz", 3, False), (src, "out.fq.bgz", ts.HOCO | ts.FASTQ, False), (src, "out.fa", 8, False), (src, "out.txt", 0, False), (src, "out.gz", 0, False),
              (src, "out.bin.gz", 0, False), (str(tmp_path / "missing.fa"), "o.fa.gz", 0, False)]
    with mg.knobs(TEXT_WINDOW_KB=kb, BGZF_BLOCK=999):
        for path, name, flags, earlier in cases:
            said = []
            for call in (mg.seq_convert_file, mg.seqconvert_file_bgzf):
                dst = str(tmp_path / name)
                if earlier:
                    open(dst, "wb").write(b"what an earlier call left")
                with pytest.raises(mg.ModgpuError) as e:
                    call(path, dst, flags)
                assert not os.path.exists(dst), (path, name, flags)
                said.append((str(e.value).split("failed: ", 1)[1], e.value.err, e.value.result))
            assert said[0] == said[1], (path, name, flags)
    # the type from the suffix before .gz and before .bgz
    with mg.knobs(BGZF_BLOCK=999):
        for name, out_type in (("a.fa.gz", 1), ("a.fq.bgz", 2), ("a.fq", 2), ("a.fa.bgz", 1)):
            dst = str(tmp_path / name)
            _, res = mg.seqconvert_file_bgzf(src, dst, 0)
            assert res["outType"] == out_type and open(dst, "rb").read().endswith(mg.BGZF_EOF)


@pytest.mark.parametrize("block", [999, 65280])
def test_bgzf_in_bgzf_out(block, tmp_path):
    """the text is inflated on the device, rewritten there and deflated there: neither the input's text nor the output's crosses the link"""
    for name, flags in (("conv_long.fa", ts.FASTQ), ("conv_many.fq", ts.FASTA), ("conv_hoco.fa", ts.HOCO)):
        data = open(os.path.join(ts.GOLDEN, name), "rb").read()
        src, dst = str(tmp_path / (name + ".gz")), str(tmp_path / "out.gz")
        open(src, "wb").write(mg.bgzf_bytes(data, block=700))
        want = ts.restate(data, flags)
        for kb in WINDOWS:
            with mg.knobs(BGZF_BLOCK=block, TEXT_WINDOW_KB=kb):
                err, res = mg.seqconvert_file_bgzf(src, dst, flags)
                assert mg.inflate_diag()["members"] > 0
                assert mg.deflate_diag()["launches"] >= 1
            got = open(dst, "rb").read()
            assert (gzip.decompress(got), err, res) == want, (name, kb)
            assert got == host_file(want[0], block), (name, kb)
