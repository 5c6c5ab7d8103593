"""Ordinary gzip through the host compile of the device's pipeline (mgGunzipHost over csrc/mg_gunzip_core.h: finder, speculative chunks, chain,
windows, resolve, members), against zlib.

The corpus below is also what tests/test_gpu_gunzip.py puts through the kernels and what tools/gunzip_host_check.c runs under the sanitizers
(write_corpus).  Every case is a whole gzip file; for a corrupt one zlib's verdict is the yardstick: where zlib refuses, the status is non-zero and
nothing outside the output range is written, where it accepts, the bytes are equal.  Every case is crossed with the chunk sizes, batch sizes and
capacity guesses of KNOBS."""
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

import modimizer_amd as mg
from tests.test_inflate_host import fasta_text, fastq_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = 1500000
CHUNKS = (4096, 16384, 32768)
BATCHES = (3, 64)
# the guess of the symbols a chunk writes: its compressed bytes (ratio 1: every text below overflows it), or 64 times as many
KNOBS = [(c, b, r) for c in CHUNKS for b in BATCHES for r in (1, 64)]


# ---------------------------------------------------------------------------------------------------------------- gzip members by hand
def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, extra=None, name=None, comment=None, hcrc=False, payload=None):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 255])
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    body = raw_deflate(data, level, strategy, mem_level) if payload is None else payload
    return head + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def zlib_verdict(blob):
    """the text if zlib (gzip wrapper, member after member to the file's last byte) accepts the file, else None"""
    out, data = [], bytes(blob)
    while True:
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(data))
        except zlib.error:
            return None
        if not d.eof:
            return None
        data = d.unused_data
        if not data:
            return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------- the corpus
def case(name, blob, text):
    return dict(name=name, blob=bytes(blob), text=text)


_GOOD = None


def good_corpus():
    global _GOOD
    if _GOOD is not None:
        return _GOOD
    fq, fa = fastq_text(TEXT, 11), fasta_text(TEXT, 12)
    out = []
    for level in (1, 6, 9):
        out.append(case("fq_l%d" % level, member(fastq_text(TEXT, level), level), fastq_text(TEXT, level)))
    out.append(case("fa_l6", member(fa), fa))
    out.append(case("fq_fixed", member(fq, 6, zlib.Z_FIXED), fq))                          # no dynamic block: nothing is found, one chain
    out.append(case("fq_level0", member(fq, 0), fq))
    noise = random.Random(13).randbytes(200000)
    mixed = fq[:600000] + noise + fa[:600000]
    out.append(case("text_noise_text", member(mixed), mixed))                               # stored blocks mid-stream
    inner = member(fq[:1200000])
    out.append(case("gzip_in_level0", member(inner, 0), inner))                             # real block headers inside stored payload: false candidates
    poly = b">polyA\n" + b"A" * TEXT + b"\n"
    out.append(case("poly_a", member(poly, 9), poly))                                       # ratio near 1000:1
    out.append(case("short_text", member(fq[:20000]), fq[:20000]))                          # less than a window
    out.append(case("one_byte", member(b"A"), b"A"))
    out.append(case("empty_member", member(b""), b""))
    for ml in (1, 3):                                                                       # blocks of 128 / 512 symbols: chunks that write less than a window
        out.append(case("fq_memlevel%d" % ml, member(fq[:400000], 6, mem_level=ml), fq[:400000]))
    a, b, c = fq[:500000], fa[:333333], fq[700000:1100001]
    out.append(case("two_members", member(a) + member(b, 9), a + b))
    out.append(case("three_members_one_empty", member(a, 1) + member(b"") + member(c), a + c))
    tiny = [fq[i:i + 999] for i in range(0, 30000, 999)]
    out.append(case("tiny_members", b"".join(member(t) for t in tiny), b"".join(tiny)))
    out.append(case("header_fields", member(a, extra=b"XY\x03\x00abc", name=b"reads.fq", comment=b"made by hand", hcrc=True), a))
    out.append(case("header_extra", member(b, extra=b"AB\x00\x00"), b))
    out.append(case("header_name", member(b, name=b"x" * 5000), b))                         # a header longer than the stream's first look
    out.append(case("header_comment_hcrc", member(b, comment=b"c", hcrc=True), b))
    _GOOD = out
    return out


_BAD = None


def corrupt_corpus():
    """files that are wrong somewhere, or look it; the verdict is zlib's"""
    global _BAD
    if _BAD is not None:
        return _BAD
    fq = fastq_text(300000, 14)
    good = member(fq)
    out = []
    crc = struct.pack("<I", zlib.crc32(fq) ^ 0x100)
    out.append(case("wrong_crc", good[:-8] + crc + good[-4:], None))
    out.append(case("wrong_isize", good[:-4] + struct.pack("<I", len(fq) + 1), None))
    out.append(case("junk_after_trailer", good + b"junk that is no header", None))
    out.append(case("junk_between_members", good + b"\x1f\x8b\x07" + good, None))
    out.append(case("reserved_flag", good[:3] + b"\x20" + good[4:], None))
    out.append(case("wrong_hcrc", member(fq, hcrc=True)[:10] + b"\0\0" + member(fq, hcrc=True)[12:], None))
    out.append(case("not_gzip", fq[:5000], None))
    out.append(case("no_bytes", b"", None))
    rng = random.Random(15)
    for i in range(20):
        at = [1, 9, 10, 11, len(good) - 1, len(good) - 4, len(good) - 8, len(good) - 9][i] if i < 8 else rng.randrange(12, len(good) - 9)
        out.append(case("cut_%02d_at_%d" % (i, at), good[:at], None))
    for i in range(50):
        at = rng.randrange(len(good)) if i >= 6 else (3, 4, 9, len(good) - 1, len(good) - 5, 10)[i]
        flipped = bytearray(good); flipped[at] ^= 1 << rng.randrange(8)
        out.append(case("flip_%02d_at_%d" % (i, at), flipped, None))
    _BAD = out
    return out


def cap_of(m):
    return len(m["text"]) if m["text"] is not None else 300000 + 4096


def write_corpus(path, knobs=KNOBS):
    """the corpus as tools/gunzip_host_check.c reads it: a count, then per run chunk bytes, batch chunks, symbols per chunk, the output's capacity and the
    file's length (little-endian words) and the file.  Returns the runs [(case, chunk, batch, symbols)]"""
    runs = [(m, c, b, c * r) for m in good_corpus() + corrupt_corpus() for (c, b, r) in knobs]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(runs)))
        for m, c, b, s in runs:
            f.write(struct.pack("<IIIII", c, b, s, cap_of(m), len(m["blob"])) + m["blob"])
    return runs


# ---------------------------------------------------------------------------------------------------------------- tests
def run(m, chunk, batch, ratio, cap=None):
    return mg.gunzip_host(m["blob"], chunk, batch, chunk * ratio, cap_of(m) if cap is None else cap)


@pytest.mark.parametrize("m", good_corpus(), ids=lambda m: m["name"])
def test_good_file_inflates_to_zlibs_bytes(m):
    assert zlib_verdict(m["blob"]) == m["text"], "the corpus itself: zlib does not accept this file"
    for chunk, batch, ratio in KNOBS:
        status, text, d, intact = run(m, chunk, batch, ratio)
        what = (m["name"], chunk, batch, ratio, d)
        assert status == 0, (mg.GUNZIP_STATUS[status],) + what
        assert text == m["text"] and intact, what
        assert d["confirmed"] == d["speculated"] - d["folded"] - d["discarded"] and d["launches"] == 4 * d["batches"], what
        assert d["batches"] >= d["members"] >= 1 and d["confirmed"] >= 1, what


@pytest.mark.parametrize("level", [1, 6, 9])
def test_zlibs_output_confirms_whole(level):
    """on zlib's own dynamic blocks the finder has no false candidate: no chunk is discarded, whatever the knobs"""
    m = [c for c in good_corpus() if c["name"] == "fq_l%d" % level][0]
    for chunk, batch, ratio in KNOBS:
        d = run(m, chunk, batch, ratio)[2]
        assert d["discarded"] == 0 and d["confirmed"] == d["speculated"] - d["folded"], (chunk, batch, ratio, d)
        if chunk == 4096 and ratio == 64:
            assert d["folded"] > 0, d                       # blocks of about 20 KiB: most chunks of 4 KiB hold no block start
        if ratio == 1:
            assert d["retries"] > 0, d                      # (the text is about twice its compressed bytes)
        if ratio == 64 and batch == 64:
            assert d["retries"] == 0 and d["batches"] <= 6, d


def by_name(name):
    return [c for c in good_corpus() if c["name"] == name][0]


def test_no_dynamic_block_is_one_chain():
    for name in ("fq_fixed", "fq_level0"):
        for chunk, batch, ratio in KNOBS:
            d = run(by_name(name), chunk, batch, ratio)[2]
            assert d["discarded"] == 0 and d["folded"] == d["speculated"] - d["confirmed"], (name, d)
            assert d["confirmed"] == d["batches"] - d["retries"], (name, d)      # nothing found: every batch is its first chunk running through


def test_false_candidates_break_the_chain_and_recover():
    """a gzip file stored in a level-0 gzip file: the inner file's block headers are byte-aligned in stored payload, the finder verifies them, and the
    chain, which walks the stored blocks, does not end on them"""
    m = by_name("gzip_in_level0")
    worst = 0
    for chunk, batch, ratio in KNOBS:
        status, text, d, intact = run(m, chunk, batch, ratio)
        assert status == 0 and text == m["text"] and intact
        worst = max(worst, d["discarded"])
    assert worst > 0


def test_capacity_retries_on_poly_a():
    m = by_name("poly_a")
    for chunk, batch, ratio in KNOBS:
        status, text, d, intact = run(m, chunk, batch, ratio)
        assert status == 0 and text == m["text"] and intact
        if ratio == 1:
            assert d["retries"] >= 6, (chunk, batch, ratio, d)      # 1.5 M symbols from one chunk of at most 32 Ki: the room doubles six times at least


def test_windows_shorter_than_32k():
    """text shorter than a window, and chunks that write less than a window each, so that a window is built from two or more chunks"""
    assert run(by_name("short_text"), 4096, 64, 64)[1] == by_name("short_text")["text"]
    m = by_name("fq_memlevel1")
    status, text, d, intact = run(m, 4096, 64, 64)
    assert status == 0 and text == m["text"]
    assert d["confirmed"] > 2 * len(m["text"]) // 32768, d


def test_member_boundaries_inside_chunks():
    for name, members in (("two_members", 2), ("three_members_one_empty", 3), ("tiny_members", 31)):
        for chunk, batch, ratio in KNOBS:
            status, text, d, intact = run(by_name(name), chunk, batch, ratio)
            assert status == 0 and text == by_name(name)["text"] and d["members"] == members, (name, d)


def check_against_zlib(m):
    want = zlib_verdict(m["blob"])
    accepted = 0
    for chunk, batch, ratio in KNOBS:
        status, text, d, intact = run(m, chunk, batch, ratio)
        assert intact, "%s: bytes outside the output range were written" % m["name"]
        if want is None:
            assert status != 0, "%s: zlib refuses this file (%d %d %d)" % (m["name"], chunk, batch, ratio)
        else:
            assert status == 0 and text == want, "%s: zlib accepts this file (%s)" % (m["name"], mg.GUNZIP_STATUS[status])
            accepted = 1
    return accepted


@pytest.mark.parametrize("m", corrupt_corpus()[:-50], ids=lambda m: m["name"])
def test_corrupt_file_gets_zlibs_verdict(m):
    assert check_against_zlib(m) == 0


def test_single_bit_flips_get_zlibs_verdict():
    accepted = sum(check_against_zlib(m) for m in corrupt_corpus()[-50:])
    assert 0 < accepted < 50                               # (a flip in MTIME or OS changes nothing)


EXPECTED_STATUS = dict(wrong_crc=8, wrong_isize=7, junk_after_trailer=10, junk_between_members=10, reserved_flag=10, wrong_hcrc=10, not_gzip=10, no_bytes=10,
                       cut_00_at_1=1, cut_02_at_10=1)


def test_each_refusal_has_its_own_status():
    cases = {m["name"]: m for m in corrupt_corpus()}
    for name, want in EXPECTED_STATUS.items():
        assert run(cases[name], 16384, 64, 64)[0] == want, name


def test_output_capacity_is_respected():
    m = by_name("fq_l6")
    for cap in (0, 1, 40000, len(m["text"]) - 1):
        for chunk, batch, ratio in ((4096, 3, 1), (32768, 64, 64)):
            status, text, d, intact = run(m, chunk, batch, ratio, cap)
            assert status == 7 and intact and m["text"].startswith(text), (cap, status)


def test_guard_page_program_agrees_over_the_corpus(tmp_path):
    """tools/gunzip_host_check.c: the core header alone, in a process of its own, every file and its output between inaccessible pages.  Its statuses
    and lengths are the library's.  (The same program is what runs under the sanitizers: its head comment has the command.)"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe, corpus = str(tmp_path / "gunzip_host_check"), str(tmp_path / "corpus.bin")
    build = subprocess.run([cc, "-O2", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "modimizer_amd", "csrc"),
                            os.path.join(ROOT, "tools", "gunzip_host_check.c"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    runs = write_corpus(corpus, [(4096, 3, 1), (16384, 64, 64)])
    got = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-4000:]
    lines = [ln.split() for ln in got.stdout.splitlines() if ln.startswith("run") and "status" in ln]
    assert len(lines) == len(runs)
    for ln, (m, c, b, s) in zip(lines, runs):
        status, text, d, _ = mg.gunzip_host(m["blob"], c, b, s, cap_of(m))
        assert (int(ln[3]), int(ln[5]), int(ln[7], 16)) == (status, len(text), zlib.crc32(text)), (m["name"], c, b, s)
        assert [int(x) for x in ln[9:17]] == [d[k] for k in mg.GUNZIP_DIAG], m["name"]


def test_example_compiles_and_the_knobs_are_read(tmp_path):
    """examples/gunzip_file.c against include/modgpu.h alone: plain C99, warnings on"""
    libdir = os.path.join(ROOT, "modimizer_amd")
    mg.lib()
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "gunzip_file.c"),
                        "-o", str(tmp_path / "gunzip_file"), "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    knobs = open(os.path.join(mg.CSRC, "mg_knobs.c")).read()
    for k in ("HOST", "CHUNK_KB", "BATCH", "RATIO", "MIN_KB"):
        assert "MODGPU_GZIP_" + k in knobs
