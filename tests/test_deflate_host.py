"""The BGZF encoder of csrc/mg_deflate_core.h through its host compile (mgDeflateBlockHost): no GPU.  Every member must be what zlib and
the project's own decoder inflate back to the block; the sizes are held against zlib's own -- Z_HUFFMAN_ONLY and level 1 over the same
65280-byte blocks -- never against the encoder's earlier output.  The corpus below is also what tests/test_gpu_deflate.py puts through the
kernel (which must write the same bytes) and what tools/deflate_host_check.c runs between guard pages (tools/asan_deflate.sh: under the
host sanitizers)."""
import functools
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import modimizer_amd as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 65280
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")      # then BSIZE


def rand_bytes(n, seed):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def dna(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(seed).randint(0, 4, n)].tobytes()


def fibonacci_text():
    """40 symbols: 22 whose counts are the Fibonacci numbers 1, 1, 2, 3 .. 17711 -- all that a block has room for -- and 18 with 1000 each, 64367
    bytes, shuffled.  Below 1000 the running sum of Fibonacci counts stays under the next but one, so a minimum-redundancy code chains the 16
    rarest symbols one below the other (the encoder breaks a tie towards the deeper tree): more than 15 bits deep, the limit has to act"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    counts = fib + [1000] * 18
    assert len(counts) == 40 and sum(counts) <= BLOCK
    t = np.repeat(np.arange(40, dtype=np.uint8) + 48, counts)
    np.random.RandomState(11).shuffle(t)
    return t.tobytes()


@functools.lru_cache(maxsize=None)
def edge_corpus():
    """[(name, text)]: the smallest shapes at which the encoder can go wrong, each at most one block"""
    half = rand_bytes(32769, 3)
    one_literal = b"q" * 5000
    return [("empty", b""), ("one_byte", b"x"), ("two_equal", b"zz"), ("equal_65280", b"A" * BLOCK), ("random_65280", rand_bytes(BLOCK, 1)),
            ("dna_65280", dna(BLOCK, 2)), ("period_32768", (half[:32768] * 2)[:BLOCK]), ("period_32769", (half * 2)[:BLOCK]),
            ("fibonacci_40", fibonacci_text()), ("one_literal_and_matches", one_literal), ("all_256", bytes(range(256))),
            ("text_4097", (b"the quick brown fox jumps over the lazy dog, " * 100)[:4097])]


def fastq_text(read_len, total, seed):
    """reads drawn at random positions from a 200 kb iid genome, headers @read%d/ccs len=%d, quality strings that keep their symbol with
    probability 0.9 and otherwise draw from 8 symbols"""
    rng = np.random.RandomState(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, 200000)]
    symbols = np.frombuffer(b"#+5:?DIF", np.uint8)
    out, size, i = [], 0, 0
    while size < total:
        at = rng.randint(0, len(genome) - read_len)
        change = rng.random_sample(read_len) >= 0.9
        change[0] = True
        draws = symbols[rng.randint(0, 8, read_len)]
        qual = draws[np.maximum.accumulate(np.where(change, np.arange(read_len), 0))]
        rec = b"@read%d/ccs len=%d\n" % (i, read_len) + genome[at:at + read_len].tobytes() + b"\n+\n" + qual.tobytes() + b"\n"
        out.append(rec); size += len(rec); i += 1
    return b"".join(out)


def fasta_text(total, seed):
    seq = dna(total, seed)
    return b">chr1 iid\n" + b"".join(seq[i:i + 70] + b"\n" for i in range(0, len(seq), 70))


@functools.lru_cache(maxsize=None)
def long_corpus():
    """[(name, text, is FASTQ)]: several blocks each"""
    return [("fastq_150", fastq_text(150, 330000, 5), True), ("fastq_10k", fastq_text(10000, 330000, 6), True), ("fasta_iid", fasta_text(190000, 7), False)]


def blocks_of(text):
    return [text[i:i + BLOCK] for i in range(0, len(text), BLOCK)] or [b""]


def raw_deflate(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def zlib_sizes(text):
    """(H, L1): the raw-deflate bytes of the text's blocks with Z_HUFFMAN_ONLY and with level 1"""
    bl = blocks_of(text)
    return (sum(len(raw_deflate(b, 6, zlib.Z_HUFFMAN_ONLY)) for b in bl), sum(len(raw_deflate(b, 1, zlib.Z_DEFAULT_STRATEGY)) for b in bl))


@functools.lru_cache(maxsize=None)
def encoded(name):
    """[(block, member, stats, guards intact)] of a corpus text, by the host compile: computed once, shared by the tests"""
    text = {n: t for n, t in edge_corpus()}.get(name) or {n: t for n, t, _ in long_corpus()}.get(name) or b""
    return [(b,) + mg.deflate_block_host(b) for b in blocks_of(text)]


def write_corpus(path):
    """the corpus as tools/deflate_host_check.c reads it: a count, then per block its length (a little-endian word) and its bytes"""
    bl = [b for name, _ in edge_corpus() for b in blocks_of(dict(edge_corpus())[name])] + [b for _, t, _ in long_corpus() for b in blocks_of(t)]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(bl)))
        for b in bl:
            f.write(struct.pack("<I", len(b)) + b)
    return bl


ALL_NAMES = [n for n, _ in edge_corpus()] + [n for n, _, _ in long_corpus()]


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", ALL_NAMES)
def test_member_round_trips_through_zlib_and_the_own_decoder(name):
    for block, member, stats, intact in encoded(name):
        assert intact, "bytes outside the 65536-byte slot were written, or the text was"
        assert len(member) <= 65536
        assert member[:16] == HEADER and struct.unpack_from("<H", member, 16)[0] == len(member) - 1
        d = zlib.decompressobj(31)
        assert d.decompress(member) == block and d.eof and d.unused_data == b""
        crc, isize = struct.unpack_from("<II", member, len(member) - 8)
        assert (crc, isize) == (zlib.crc32(block), len(block))
        status, text, _, ok = mg.inflate_member_host(member[18:-8], len(block), crc)
        assert status == 0 and text == block and ok, mg.INFLATE_STATUS[status]
        assert (stats["bits"] + 7) // 8 == len(member) - 26 and stats["distance"] <= 32768 and stats["match"] <= 258
        assert stats["literals"] + stats["matches"] <= max(len(block), 0) and (stats["kind"] == 2) == (stats["matches"] > 0)


def test_edge_corpus_takes_the_paths_it_is_there_for():
    st = {name: encoded(name)[0][2] for name, _ in edge_corpus()}
    assert st["random_65280"]["kind"] == 0 and len(encoded("random_65280")[0][1]) == BLOCK + 5 + 26
    assert st["dna_65280"]["kind"] in (1, 2) and len(encoded("dna_65280")[0][1]) < BLOCK // 3
    e = st["equal_65280"]
    assert (e["kind"], e["match"], e["distance"], e["dist_bits"], e["literals"]) == (2, 258, 1, 1, 1) and e["matches"] == -(-(BLOCK - 1) // 258)
    assert st["period_32768"]["kind"] == 2 and st["period_32768"]["distance"] == 32768 and st["period_32768"]["match"] == 258
    assert st["period_32769"]["kind"] == 0 and st["period_32769"]["matches"] == 0      # the only repeat lies one byte too far: nothing may reach it
    assert st["fibonacci_40"]["litlen_bits"] == 15 and st["fibonacci_40"]["kind"] == 1
    assert st["one_literal_and_matches"]["kind"] == 2 and st["one_literal_and_matches"]["literals"] == 1
    assert st["two_equal"]["matches"] == 0 and st["empty"]["matches"] == 0 and st["one_byte"]["literals"] == 1
    assert st["all_256"]["kind"] == 0                           # nothing to gain: stored
    assert {s["kind"] for s in st.values()} == {0, 1, 2}
    assert max(s["match"] for s in st.values()) == 258 and max(s["distance"] for s in st.values()) == 32768


@pytest.mark.parametrize("name", ALL_NAMES)
def test_never_larger_than_zlibs_huffman_only(name):
    """the encoder can always choose literals only, a Huffman code of the same histogram as zlib's: 1 % for ties, the 15-bit repair and the header's runs"""
    text = b"".join(b for b, _, _, _ in encoded(name))
    ours = sum(len(m) - 26 for _, m, _, _ in encoded(name))
    h, l1 = zlib_sizes(text)
    print("%s: %d text bytes, ours %d, zlib Huffman-only %d (ours / H = %.4f), level 1 %d" % (name, len(text), ours, h, ours / max(h, 1), l1))
    assert ours <= h * 1.01


@pytest.mark.parametrize("name", [n for n, _, fq in long_corpus() if fq])
def test_fastq_gains_at_least_half_of_what_level_1_gains(name):
    """first the reference alone: matches must be worth something on this text (H >= 1.3 L1); then ours is at most half way between the two"""
    text = b"".join(b for b, _, _, _ in encoded(name))
    ours = sum(len(m) - 26 for _, m, _, _ in encoded(name))
    h, l1 = zlib_sizes(text)
    print("%s: H / L1 = %.3f, ours %d, (H + L1) / 2 = %d" % (name, h / l1, ours, (h + l1) // 2))
    assert h >= 1.3 * l1
    assert ours <= (h + l1) / 2
    assert any(s["kind"] == 2 for _, _, s, _ in encoded(name))


def test_a_member_is_a_function_of_its_bytes_alone():
    """the same block at another address and beside other bytes gives the same member"""
    block = long_corpus()[0][1][1000:1000 + 5003]
    a = mg.deflate_block_host(block, guard=64)[0]
    b = mg.deflate_block_host(block, guard=77)[0]
    assert a == b and a == mg.deflate_block_host(bytes(bytearray(block)))[0]


def test_refusals_and_names():
    out = np.zeros(65536, np.uint8)
    n = mg.C.c_uint32(7)
    big = np.zeros(BLOCK + 1, np.uint8)
    assert mg.lib().mgDeflateBlockHost(big.ctypes.data, BLOCK + 1, out.ctypes.data, mg.C.byref(n), None) == -1 and n.value == 0
    assert b"65280" in mg.lib().mgLastError()
    assert mg.lib().mgDeflateBlockHost(None, 5, out.ctypes.data, mg.C.byref(n), None) == -1
    header = open(os.path.join(ROOT, "include", "modgpu.h")).read()
    for name in ("mgDeflateBlocksDevice", "mgDeflateBlockHost", "mgDeflateDiag", "mgBgzfDeflateFile", "mgSeqConvertFileBgzf"):
        assert name in mg.EXPORTS and hasattr(mg.lib(), name) and (name + " (") in header, name
    assert "} MgGzBlock;" in header and mg.C.sizeof(mg.MgGzBlock) == 16
    for f in ("deflate_blocks_device", "deflate_block_host", "deflate_diag", "bgzf_deflate_file", "seqconvert_file_bgzf"):
        assert callable(getattr(mg, f)), f
    mk = open(os.path.join(mg.CSRC, "Makefile")).read()
    assert "mg_deflate.o" in mk and "mg_bgzfsink.o" in mk and "mg_deflate_core.h" in mk
    assert "MODGPU_BGZF_BLOCK" in open(os.path.join(mg.CSRC, "mg_knobs.c")).read()
    assert mg.BGZF_EOF == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def test_example_compiles(tmp_path):
    """examples/deflate_file.c against include/modgpu.h alone: plain C99, warnings on"""
    libdir = os.path.join(ROOT, "modimizer_amd")
    mg.lib()
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "deflate_file.c"),
                        "-o", str(tmp_path / "deflate_file"), "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_guard_page_program_agrees_over_the_corpus(tmp_path):
    """tools/deflate_host_check.c: the encoder alone, in a process of its own, every block between inaccessible pages that end (then begin) exactly at
    the text, the slot and the token list.  Its members are the library's.  (tools/asan_deflate.sh builds the same program with the sanitizers.)"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe, corpus = str(tmp_path / "deflate_host_check"), str(tmp_path / "corpus.bin")
    build = subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "modimizer_amd", "csrc"),
                            os.path.join(ROOT, "tools", "deflate_host_check.c"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    blocks = write_corpus(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("block") and " crc " in ln]
    assert len(lines) == len(blocks)
    want = [(m, s) for name in ALL_NAMES for _, m, s, _ in encoded(name)]
    for ln, b, (member, stats) in zip(lines, blocks, want):
        assert (int(ln[3]), int(ln[5], 16), int(ln[7])) == (len(member), zlib.crc32(member), stats["kind"]), ln
