"""modasm's read ingest (readsetFileRead + invBuild + readsetStats + the .readset file): oracle and
GPU path against the reference program's own output (tests/golden/asm_*: modutils -c 20 k w 17 -a reads.fa
-s 2 3 5 -w src.mod; modasm -m src.mod -f reads2.fa -S -w stem)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import fasta
from tests import util

TAGS = {"k21d16": (21, 16), "k17d31": (17, 31)}


def readset_mask(raw):
    """.readset bytes with the in-memory addresses (Array.base, Read.hit, Read.dx) zeroed"""
    b = bytearray(raw)
    at = 16
    b[at + 8:at + 16] = bytes(8)
    dim = int.from_bytes(b[at + 16:at + 20], "little")
    size = int.from_bytes(b[at + 20:at + 24], "little")
    assert size == 72
    at += 32
    for i in range(dim):
        b[at + 72 * i + 8:at + 72 * i + 24] = bytes(16)
    return bytes(b)


def mod_mask(raw, bits=20):
    b = bytearray(raw)
    at = 8 + 4 + 4 + 8 + 80 + 4 * (1 << bits)
    b[at:at + 8] = bytes(8)                          # value[0]: never initialised by the reference
    return bytes(b)


def rs_lines(text):
    return [l for l in text.splitlines() if l.startswith("RS ")]


@pytest.mark.parametrize("tag", list(TAGS))
def test_oracle_readset_vs_reference_program(tag, golden_dir, tmp_path):
    from oracle import pyoracle as orc
    k, w = TAGS[tag]
    h = orc.Hasher(k, w, 17)
    ms = orc.Modset(h, 20)
    for s in fasta.read_fasta_list(os.path.join(golden_dir, "reads.fa")):
        ms.add_sequence(s)
    ms.set_copy(2, 3, 5)
    p = str(tmp_path / "src.mod"); ms.write_mod(p)
    assert mod_mask(open(p, "rb").read()) == mod_mask(gzip.open(os.path.join(golden_dir, "asm_%s_src.mod" % tag)).read())
    rs = orc.Readset(ms)
    rs.read(fasta.read_fasta_list(os.path.join(golden_dir, "reads2.fa")))
    assert rs_lines(rs.stats_text(str(tmp_path / "s.txt"))) == rs_lines(util.golden_text("asm_%s.stdout.txt" % tag))
    out = str(tmp_path / "o.readset"); rs.write(out)
    assert readset_mask(open(out, "rb").read()) == readset_mask(gzip.open(os.path.join(golden_dir, "asm_%s.readset" % tag)).read())
    ms.write_mod(p)                                  # depth rebuilt from the reads (modasm.c:158,174)
    assert mod_mask(open(p, "rb").read()) == mod_mask(gzip.open(os.path.join(golden_dir, "asm_%s.mod" % tag)).read())
    a = rs.arrays()
    # inverse lists: per mod, the reads that hit it, in read order, one entry per hit
    d = ms.depths()
    assert int(a["invStart"][-1]) == int(d[(d > 0) & (d < 65535)].sum()) == a["totHit"]
    for i in np.flatnonzero(d[1:] > 0)[:200] + 1:
        got = a["invSpace"][int(a["invStart"][i]):int(a["invStart"][i]) + int(d[i])]
        want = [r + 1 for r in range(len(a["nHit"])) for hh in a["hit"][int(a["hitStart"][r]):int(a["hitStart"][r + 1])]
                if (int(hh) & 0x7fffffff) == i]
        assert list(got) == want
    rs.close(); ms.close()


# ---- the library (mg_readset.c; the passes in mg_rs_clean.c, mg_rs_overlap.c, mg_rs_rdna.c have test files of their own) ----

def lib_arrays(rs):
    r = rs.contents
    n, tot, m = r.nReads, int(r.totHit), r.ms.contents.max
    as_np = lambda p, k, dt, off=0: np.ctypeslib.as_array(p, (max(k + off, 1),))[off:k + off].astype(dt).copy()
    return {"len": as_np(r.len, n, np.int64, 1), "nHit": as_np(r.nHit, n, np.int64, 1), "nMiss": as_np(r.nMiss, n, np.int64, 1),
            "nCopy": np.array([list(r.nCopy[i]) for i in range(1, n + 1)]).reshape(n, 4),
            "hitStart": as_np(r.hitStart, n + 1, np.uint64, 1), "hit": as_np(r.hit, tot, np.uint32),
            "dx": as_np(r.dx, tot, np.uint16), "totHit": tot,
            "invStart": as_np(r.invStart, m + 2, np.uint64), "invSpace": as_np(r.invSpace, int(r.invStart[m + 1]), np.uint32)}


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def stats_text(rs, tmp):
    with mg.CFile(tmp, "w") as f:
        mg.lib().mgReadsetStats(rs, f)
    return open(tmp).read()


@pytest.mark.parametrize("tag", list(TAGS))
def test_load_write_readset_files(tag, golden_dir, tmp_path):
    """the reference's own <stem>.mod + <stem>.readset: load, print the stats, write back the same bytes"""
    L = mg.lib()
    stem = os.path.join(golden_dir, "asm_%s" % tag)
    rs = L.mgReadsetLoad(stem.encode())
    assert rs.contents.nReads == 82
    got = stats_text(rs, str(tmp_path / "s.txt")).splitlines()
    assert got == util.golden_text("asm_%s.stdout.txt" % tag).splitlines()[-len(got):] and len(got) == 9
    out = str(tmp_path / "again")
    L.mgReadsetWrite(rs, out.encode())
    assert gzip.open(out + ".mod").read() == gzip.open(stem + ".mod").read()
    assert readset_mask(gzip.open(out + ".readset").read()) == readset_mask(gzip.open(stem + ".readset").read())
    rs2 = L.mgReadsetLoad(out.encode())
    same(lib_arrays(rs), lib_arrays(rs2))
    L.mgReadsetDestroy(rs); L.mgReadsetDestroy(rs2)


def load_mod_gz(path, tmp):
    open(tmp, "wb").write(gzip.open(path).read())
    with mg.CFile(tmp, "r") as f:
        return mg.lib().modsetRead(f)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAGS))
def test_readset_file_read_gpu(tag, golden_dir, tmp_path):
    """modasm -m src.mod -f reads2.fa -S -w stem with the scan + lookups on the GPU: same statistics,
    same .readset and .mod bytes (depth rebuilt from the reads)"""
    L = mg.lib()
    ms = load_mod_gz(os.path.join(golden_dir, "asm_%s_src.mod" % tag), str(tmp_path / "src.mod"))
    rs = L.mgReadsetCreate(ms)
    os.environ["MODGPU_FILE_BATCH_MBP"] = "1"; L.mgReloadKnobs()        # several batches: reads2.fa holds 120 kb... one batch; the knob is exercised below
    try:
        assert L.mgReadsetFileRead(rs, os.path.join(golden_dir, "reads2.fa").encode()) == 0
    finally:
        del os.environ["MODGPU_FILE_BATCH_MBP"]; L.mgReloadKnobs()
    got = stats_text(rs, str(tmp_path / "s.txt")).splitlines()
    assert got == util.golden_text("asm_%s.stdout.txt" % tag).splitlines()[-len(got):]
    out = str(tmp_path / "gpu")
    L.mgReadsetWrite(rs, out.encode())
    stem = os.path.join(golden_dir, "asm_%s" % tag)
    assert mod_mask(gzip.open(out + ".mod").read()) == mod_mask(gzip.open(stem + ".mod").read())
    assert readset_mask(gzip.open(out + ".readset").read()) == readset_mask(gzip.open(stem + ".readset").read())
    L.mgReadsetDestroy(rs)


def saturation_case(tmp_path):
    """eight reads and an oracle modset, written to a .mod file: a k-mer hit more than 65535 times, an empty and a short read, both strands"""
    from oracle import pyoracle as orc
    rng = np.random.default_rng(11)
    k, w = 15, 1
    g = rng.integers(0, 4, 30000).astype(np.uint8)
    reads = [np.zeros(70000, np.uint8), g[:9000], (3 - g[2000:12000][::-1]).astype(np.uint8), np.zeros(0, np.uint8),
             g[100:110], rng.integers(0, 4, 5000).astype(np.uint8), np.zeros(3000, np.uint8), g[20000:30000]]
    h = orc.Hasher(k, w, 17); oms = orc.Modset(h, 20)
    for s in (reads[0][:100], g):
        oms.add_sequence(s)
    oms.set_copy(1, 2, 3)
    p = str(tmp_path / "m.mod"); oms.write_mod(p)
    return reads, oms, p


@pytest.mark.gpu
def test_readset_vs_oracle_saturation_and_batches(tmp_path):
    """a k-mer hit more than 65535 times (depth saturates, no inverse list: modasm.c:174,266,278), empty
    and short reads, reads on both strands; the same reads in one call and through a file in batches"""
    from oracle import pyoracle as orc
    reads, oms, p = saturation_case(tmp_path)      # the same modset for the library: through a .mod file
    ors = orc.Readset(oms); ors.read(reads)
    want = ors.arrays()
    assert int(oms.depths().max()) == 65535
    L = mg.lib()
    for mode in ("memory", "file"):
        with mg.CFile(p, "r") as f:
            ms = L.modsetRead(f)
        rs = L.mgReadsetCreate(ms)
        if mode == "memory":
            bases, offs = util.concat_reads(reads)
            assert L.mgReadsetRead(rs, bases.ctypes.data, offs.ctypes.data, len(reads)) == 0
        else:
            fa = str(tmp_path / "r.fa")
            with open(fa, "w") as f:
                for i, s in enumerate(reads):
                    f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in s)))
            os.environ["MODGPU_FILE_BATCH_MBP"] = "1"
            os.environ["MODGPU_FILE_BATCH_BASES"] = "9500"; L.mgReloadKnobs()
            try:
                assert L.mgReadsetFileRead(rs, fa.encode()) == 0
            finally:
                del os.environ["MODGPU_FILE_BATCH_MBP"]; del os.environ["MODGPU_FILE_BATCH_BASES"]; L.mgReloadKnobs()
        same(want, lib_arrays(rs))
        assert np.array_equal(np.ctypeslib.as_array(ms.contents.depth, (ms.contents.max + 1,)), oms.depths())
        assert rs_lines(stats_text(rs, str(tmp_path / "s.txt"))) == rs_lines(ors.stats_text(str(tmp_path / "o.txt")))
        L.mgReadsetDestroy(rs)
    ors.close(); oms.close()


@pytest.mark.gpu
def test_readset_second_read_into_a_set_with_hits(tmp_path):
    """the same eight reads in two calls of four: the second call finds hits in the set, so depth[], the inverse lists and nCopy[] are made
    from all the hits by the host loops; checked against their definitions over the hit lists, then written, loaded (the lists made again
    from the file's depth[]) and compared"""
    reads, oms, p = saturation_case(tmp_path)
    L = mg.lib()
    with mg.CFile(p, "r") as f:
        ms = L.modsetRead(f)
    rs = L.mgReadsetCreate(ms)
    for part in (reads[:4], reads[4:]):
        bases, offs = util.concat_reads(part)
        assert L.mgReadsetRead(rs, bases.ctypes.data, offs.ctypes.data, len(part)) == 0
    a = lib_arrays(rs)
    n, m = rs.contents.nReads, ms.contents.max
    assert n == 8 and a["totHit"] > 65535
    info = np.ctypeslib.as_array(ms.contents.info, (m + 1,)).copy()
    mod = (a["hit"] & np.uint32(0x7fffffff)).astype(np.int64)
    assert mod.min() >= 1 and mod.max() <= m
    depth = np.minimum(np.bincount(mod, minlength=m + 1), 65535)
    assert depth.max() == 65535
    assert np.array_equal(np.ctypeslib.as_array(ms.contents.depth, (m + 1,)), depth)
    listed = np.where((depth > 0) & (depth < 65535), depth, 0)
    assert np.array_equal(a["invStart"], np.concatenate(([0], np.cumsum(listed))).astype(np.uint64))
    start = a["hitStart"].astype(np.int64)
    read_of = np.repeat(np.arange(1, n + 1), np.diff(start))
    keep = listed[mod] > 0
    assert keep.any() and not keep.all()
    assert np.array_equal(a["invSpace"], read_of[keep][np.argsort(mod[keep], kind="stable")])
    n_copy = np.array([np.bincount(info[mod[start[r]:start[r + 1]]] & 3, minlength=4) for r in range(n)])
    assert np.array_equal(a["nCopy"], n_copy) and (n_copy.sum(axis=0) > 0).sum() >= 2
    out = str(tmp_path / "twice")
    L.mgReadsetWrite(rs, out.encode())
    rs2 = L.mgReadsetLoad(out.encode())
    same(a, lib_arrays(rs2))
    L.mgReadsetDestroy(rs); L.mgReadsetDestroy(rs2)
    oms.close()


# ---- more than 1024 tiles of seeds in one batch: the tile scan (mgRsTileScanKernel) past one count per thread ----

RS_TILE = 4096                 # mg_chain.hip MG_RS_TILE: seeds per tile
RS_K = 15
# tiles -> seeds of the batch: a last tile that holds the end of a gap read and little more, a last tile that is exactly full, one more tile than that
RS_TILE_CASES = {1025: 1024 * RS_TILE + 4000, 2048: 2048 * RS_TILE, 2049: 2048 * RS_TILE + 4000}
_rs_shared = {}


def _rs_genome_and_mod():
    """the genome and the oracle's modset of its k-mers as .mod bytes, made once for the cases (the oracle's set itself is kept too: a read
    set zeroes its depths when it begins, modasm.c:158, and leaves the rest as it is)"""
    if not _rs_shared:
        from oracle import pyoracle as orc
        import tempfile
        g = util.without_two_letter_windows(np.random.default_rng(2024).integers(0, 4, 200_000).astype(np.uint8), RS_K)
        h = orc.Hasher(RS_K, 1, 17); oms = orc.Modset(h, 20)
        oms.add_sequence(g)
        oms.set_copy(1, 2, 3)
        with tempfile.TemporaryDirectory() as d:
            oms.write_mod(os.path.join(d, "m.mod"))
            _rs_shared.update(g=g, oms=oms, mod=open(os.path.join(d, "m.mod"), "rb").read())
    return _rs_shared["g"], _rs_shared["mod"]


def rs_tile_case(n_tiles):
    """(reads, tiles of the gap reads' second hits, tiles at whose first seed a read begins) for a batch of n_tiles tiles of seeds.
    k = 15, w = 1: every k-mer is a seed, a read of len bases has len - 14 of them, in base order.  Reads over {A, C} hit nothing."""
    g, _ = _rs_genome_and_mod()
    rng = np.random.default_rng(n_tiles)
    k, total = RS_K, RS_TILE_CASES[n_tiles]
    reads, at = [], [0]                                   # at[0]: seeds so far
    def add(r):
        reads.append(np.ascontiguousarray(r, np.uint8)); at[0] += max(len(r) - k + 1, 0)
    junk = lambda n: rng.integers(0, 2, n).astype(np.uint8)
    def cut(n):
        a = int(rng.integers(0, len(g) - n))
        return (3 - g[a:a + n][::-1]) if rng.random() < 0.5 else g[a:a + n]
    def fill_to(target):                                  # long reads that hit nothing and reads cut from g, then one that ends on the seed
        assert at[0] <= target
        while target - at[0] > 120_000:
            add(junk(int(rng.integers(20_000, 60_000))))
            add(cut(int(rng.integers(3 * RS_TILE + k, 5 * RS_TILE))))
        if target > at[0]:
            add(junk(target - at[0] + k - 1))
        assert at[0] == target
    gaps = [1024] + ([2048] if n_tiles > 2048 else [])   # the tile of the hits after the gap: tiles b - 4 .. b - 1 hold no hit
    starts = [512] + ([1536] if n_tiles >= 2048 else [])
    events = sorted([(b * RS_TILE, "start") for b in starts] + [((b - 4) * RS_TILE - 200, "gap") for b in gaps])
    for seed, what in events:
        fill_to(seed)
        add(np.zeros(0, np.uint8)); add(g[100:110])       # an empty read and one shorter than k: no seeds, directly before
        if what == "start":
            add(cut(3 * RS_TILE + 500))                   # its first seed is the tile's first seed, and a hit
        else:                                             # 186 hits, 14 seeds across the joint, 20 000 seeds that miss from the tile's first seed on, 186 hits
            a, b = (int(x) for x in rng.integers(0, len(g) - 200, 2))
            add(np.concatenate([g[a:a + 200], junk(20_000), g[b:b + 200]]))
    fill_to(total)
    return reads, gaps, starts


def rs_tile_properties(reads, want, n_tiles, gaps, starts):
    """the case holds what it claims, from the reads' lengths and the oracle's arrays"""
    k = RS_K
    seeds = np.array([max(len(r) - k + 1, 0) for r in reads], np.int64)
    seed_start = np.concatenate([[0], np.cumsum(seeds)])
    assert (int(seed_start[-1]) + RS_TILE - 1) // RS_TILE == n_tiles and int(seed_start[-1]) == RS_TILE_CASES[n_tiles]
    n_hit, hs, dx = want["nHit"].astype(np.int64), want["hitStart"].astype(np.int64), want["dx"].astype(np.int64)
    # a hit's position in its read: the sum of the read's dx so far (no distance of these reads reaches 2^16; w = 1: position = seed number)
    c = np.concatenate([[0], np.cumsum(dx)])
    read_of = np.repeat(np.arange(len(reads)), n_hit)
    pos = c[1:] - c[hs[read_of]]
    assert (pos >= 0).all() and (pos < seeds[read_of]).all()
    first = np.zeros(len(dx), bool); first[hs[:-1][n_hit > 0]] = True
    far = ~first & (dx > RS_TILE)                          # its predecessor in the same read lies more than a tile of seeds back
    assert far.sum() >= len(gaps)
    per_tile = np.bincount((seed_start[read_of] + pos) // RS_TILE, minlength=n_tiles)
    assert len(per_tile) == n_tiles and (per_tile == 0).any() and (per_tile == RS_TILE).any()
    far_tiles = set(((seed_start[read_of] + pos)[far] // RS_TILE).tolist())
    for b in gaps:                                         # four whole tiles without a hit, then the read's second hits: across the threads' pieces of the tile scan
        assert not per_tile[b - 4:b].any() and per_tile[b - 5] > 0 and b in far_tiles, b
    for b in starts:                                       # a read begins on the tile's first seed, with a hit, behind two reads without seeds
        r = int(np.searchsorted(seed_start, b * RS_TILE, side="right")) - 1
        assert seed_start[r] == b * RS_TILE and seeds[r] > 0 and seeds[r - 1] == 0 and seeds[r - 2] == 0 and len(reads[r - 2]) == 0
        assert n_hit[r] == seeds[r] and dx[hs[r]] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_tiles", list(RS_TILE_CASES))
def test_readset_past_1024_tiles_vs_oracle(n_tiles, tmp_path):
    """one batch of 1025 / 2048 / 2049 tiles of 4096 seeds: mgRsTileScanKernel's exclusive sum of the tiles' hit counts and running
    maximum of `last hit before this tile`, in place, with 2 or 3 counts per thread.  Reads that hit nothing (tiles of count 0), reads
    cut from the genome on both strands (full tiles), reads with a hit, four whole tiles without one, then a hit -- the maximum has to
    come across empty tiles and across the threads' pieces (tiles 1023 | 1024, and 2047 | 2048) --, a read whose first seed is a tile's
    first, reads without seeds before them.  dx is the reference's own 16-bit truncation (modasm.c:172)."""
    from oracle import pyoracle as orc
    _, mod = _rs_genome_and_mod()
    reads, gaps, starts = rs_tile_case(n_tiles)
    p = str(tmp_path / "m.mod"); open(p, "wb").write(mod)
    oms = _rs_shared["oms"]
    ors = orc.Readset(oms); ors.read(reads)
    want = ors.arrays()
    rs_tile_properties(reads, want, n_tiles, gaps, starts)
    L = mg.lib()
    with mg.CFile(p, "r") as f:
        ms = L.modsetRead(f)
    rs = L.mgReadsetCreate(ms)
    bases, offs = util.concat_reads(reads)
    assert L.mgReadsetRead(rs, bases.ctypes.data, offs.ctypes.data, len(reads)) == 0
    same(want, lib_arrays(rs))
    assert np.array_equal(np.ctypeslib.as_array(ms.contents.depth, (ms.contents.max + 1,)), oms.depths())
    L.mgReadsetDestroy(rs)
    ors.close()
