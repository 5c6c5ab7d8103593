"""Shared helpers for the parity tests (checker side: may use oracle/)."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

_scan = None


def scan_vectors():
    global _scan
    if _scan is None:
        _scan = np.load(os.path.join(GOLDEN, "scan_vectors.npz"))
    return _scan


def scan_configs():
    v = scan_vectors()
    return [tuple(int(x) for x in row) for row in v["configs"]]


def scan_cases(ci):
    """yield (name, bases, kmer, pos, isF) for config ci"""
    v = scan_vectors()
    for name in v["c%d_names" % ci]:
        name = str(name)
        yield (name, v["c%d_%s_in" % (ci, name)], v["c%d_%s_kmer" % (ci, name)],
               v["c%d_%s_pos" % (ci, name)], v["c%d_%s_isf" % (ci, name)])


def minimizer_case(ci, name):
    v = scan_vectors()
    key = "c%d_%s_min_hash" % (ci, name)
    if key not in v.files:
        return None
    return v[key], v["c%d_%s_min_pos" % (ci, name)], v["c%d_%s_min_isf" % (ci, name)]


def golden_text(name):
    return open(os.path.join(GOLDEN, name)).read()


def check_dump(text, golden_name):
    """compare a -wt dump with the golden full text, or with its digest (sha256 + head/tail)"""
    full = os.path.join(GOLDEN, golden_name)
    if os.path.exists(full):
        assert text == open(full).read()
        return
    dig = json.load(open(full.replace(".txt", ".digest.json")))
    lines = text.splitlines()
    assert len(lines) == dig["lines"]
    assert lines[:40] == dig["head"] and lines[-5:] == dig["tail"]
    assert hashlib.sha256(text.encode()).hexdigest() == dig["sha256"]


def concat_reads(reads):
    """list of uint8 arrays -> (bases, offsets int64)"""
    offs = np.zeros(len(reads) + 1, np.int64)
    if reads:
        offs[1:] = np.cumsum([len(r) for r in reads])
    bases = np.concatenate(reads) if reads else np.zeros(0, np.uint8)
    return bases.astype(np.uint8), offs


def without_two_letter_windows(g, k):
    """g (bases 0..3) with no window of k bases over {A, C} alone or over {G, T} alone: a sequence over {A, C} then shares no k-mer with g
    on either strand, so a test can build reads that are certain to miss"""
    g = g.copy()
    for _ in range(50):
        low = (g < 2).astype(np.int64)
        hit = False
        for run, other in ((low, 2), (1 - low, 0)):
            c = np.concatenate([[0], np.cumsum(run)])
            for s in np.flatnonzero(c[k:] - c[:-k] == k):
                g[s + k // 2] = other + (g[s + k // 2] & 1); hit = True
        if not hit:
            return g
    raise AssertionError("the sequence keeps a two-letter window")


def oracle_scan_batch(hasher, bases, offs):
    ks, ps, fs, st = [], [], [], [0]
    for r in range(len(offs) - 1):
        a, b, c = hasher.scan(bases[offs[r]:offs[r + 1]])
        ks.append(a); ps.append(b); fs.append(c); st.append(st[-1] + len(a))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return cat(ks, np.uint64), cat(ps, np.int32), cat(fs, np.uint8), np.array(st, np.int64)


MODUTILS_TAGS = {"k21d64": (20, 21, 64, 17), "k31d4": (22, 31, 4, 17), "k19d31": (20, 19, 31, 17)}
MODMAP_TAGS = {"k21d64": (21, 64), "k15d8": (15, 8), "k19d31": (19, 31)}


def bench_lines(stdout):
    """bench.py's stdout -> (the driver's line, the whole result): the LAST line is the compact one the driver parses,
    an earlier `BENCH_DETAIL {...}` line carries everything"""
    lines = stdout.splitlines()
    compact = [l for l in lines if l.startswith("{")]
    detail = [l for l in lines if l.startswith("BENCH_DETAIL ")]
    return (json.loads(compact[-1]) if compact else None, json.loads(detail[-1][len("BENCH_DETAIL "):]) if detail else None, compact)


# ------------------------------------------------------------------------------------------------
# Where a k-mer belongs in the device table: a numpy restatement of csrc/mg_common.h (mgMixBits, mgMixK, mgBucketOfM) and of the geometry
# choice in csrc/mg_table.hip (mgSetGeometry, mgSlotsFor), written from their comments and formulas.  The tests use it to craft
# k-mers that crowd one bucket and to say beforehand which geometry a table will take.

MIX_TOP = 10                    # the top bits of the mix that cost one multiply: (A ^ g (L)) : mixBits (L)
MIX_MUL = 0x9E3779B1
_M1, _M2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
U = np.uint64


def mix_bits(x, b):
    """murmur-style bijection of b-bit values (x: uint64 array)"""
    x = np.asarray(x, np.uint64)
    mask = U((1 << b) - 1)
    h = U((b + 1) >> 1)
    # modulo 2^b only the multipliers' low b bits count, so one formula serves the 32-bit form (b <= 32: 0xed558ccd, 0x1a85ec53) too
    with np.errstate(over="ignore"):
        x = x ^ (x >> h); x = (x * U(_M1)) & mask
        x = x ^ (x >> h); x = (x * U(_M2)) & mask
        x = x ^ (x >> h)
    return x


def mix_k(x, b):
    """the table's hash of a k-mer of b = 2k bits: a bijection onto b-bit values"""
    x = np.asarray(x, np.uint64)
    if b < 24:
        return mix_bits(x, b)
    lb = b - MIX_TOP
    L = x & U((1 << lb) - 1); A = x >> U(lb)
    return ((A ^ _mix_g(L, lb)) << U(lb)) | mix_bits(L, lb)


def _mix_g(L, lb):
    low = L & U((1 << min(lb, 32)) - 1)
    return ((low * U(MIX_MUL)) & U(0xffffffff)) >> U(32 - MIX_TOP)


def bucket_of(kmers, k, log2nb):
    """bucket of each k-mer in a table of 2^log2nb buckets: the top bits of its mix"""
    m = mix_k(kmers, 2 * k)
    if not log2nb:
        return np.zeros(len(m), np.uint64)
    s = 2 * k - log2nb
    return m >> U(s) if s >= 0 else (m << U(-s)) & U(0xffffffff)


def home_of(kmers, k, r):
    """home slot of each k-mer in a bucket of r slots (mgHomeOfM): the low word of its mix, stirred with the top MIX_TOP bits where the
    mix has them (2k >= 24), once more multiplied, and the high half of that times r -- so r need be no power of two"""
    b = 2 * k
    m = mix_k(kmers, b)
    w = U(0xffffffff)
    x = m & w
    if b >= 24:
        x = x ^ (((m >> U(b - MIX_TOP)) * U(0x9E5)) & w)
    x = (x * U(0x85EBCA6B)) & w
    return (x * U(r)) >> U(32)


def kmers_with_mix_prefix(rng, n, prefix, prefix_bits, k):
    """n distinct k-mers (2k >= 24) whose table hash starts with the prefix_bits <= 10 bits of `prefix`: they share a bucket in every
    table of up to 2^prefix_bits buckets, and spread evenly over the buckets below it in a larger one"""
    b = 2 * k
    assert b >= 24 and 0 <= prefix_bits <= MIX_TOP and 0 <= prefix < (1 << prefix_bits)
    lb = b - MIX_TOP
    assert n <= (1 << lb) // 2, "not that many distinct low parts"
    low = np.unique(rng.integers(0, 1 << lb, n + n // 8 + 8, dtype=np.uint64))
    assert len(low) >= n
    low = rng.permutation(low)[:n]
    free = MIX_TOP - prefix_bits
    top = (U(prefix) << U(free)) | rng.integers(0, 1 << free, n, dtype=np.uint64)
    return ((top ^ _mix_g(low, lb)) << U(lb)) | low


R_QUANTUM = 64


def table_geometry(want_slots, want_r=4096):
    """(log2 NB, R) for a table of want_slots slots: NB a power of two, at most 2^18, R the slots of a bucket, a multiple of 64 and at
    most want_r where the size allows (8192 beyond that)"""
    rmax = max(min(want_r, 8192), R_QUANTUM)
    want = max(want_slots, R_QUANTUM)
    lg = 0
    while lg < 18 and (want + (1 << lg) - 1) // (1 << lg) > rmax:
        lg += 1
    r = (want + (1 << lg) - 1) >> lg
    r = (r + R_QUANTUM - 1) // R_QUANTUM * R_QUANTUM
    return lg, min(r, 8192)


def slots_for(entries, load_pct, table_bits):
    """slots wanted for `entries` at that load: 2^16 at least, 2^(table_bits - 1) at most"""
    return min(max(entries * 100 // load_pct + 1, 1 << 16), 1 << (table_bits - 1))


LOOKUP_LOAD, BUILD_LOAD = 40, 60


def kmer_reads(hasher, kmers, k):
    """every candidate k-mer as a read of k bases (first base in the top bits), scanned with the oracle: a set built with w = 1 takes
    every k-mer start as a modimizer, and the scan emits the canonical one of a k-mer and its reverse complement.  Returns (kept,
    bases, offs): the candidates the oracle emits unchanged, in order, and their reads.  A mistake here shows as a smaller kept set
    (callers assert its size), never as an agreement of the device with itself: the device is compared with the oracle on the reads."""
    kmers = np.asarray(kmers, np.uint64)
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    bases = ((kmers[:, None] >> shifts[None, :]) & U(3)).astype(np.uint8)
    offs = np.arange(len(kmers) + 1, dtype=np.int64) * k
    got, _, _, st = oracle_scan_batch(hasher, bases.reshape(-1), offs)
    assert np.array_equal(st, np.arange(len(kmers) + 1)), "a read of k bases has one k-mer"
    keep = got == kmers
    return kmers[keep], bases[keep].reshape(-1), np.arange(int(keep.sum()) + 1, dtype=np.int64) * k


DIAG = ("log2NB", "R", "direct", "part1", "part2_16", "part2_8", "pack8", "rehash_bucket", "rehash_atomic")


def table_diag(ms):
    """mgTableDiag: the device table's geometry and, since it was made, its lookup batches by direct probes, by one partition level,
    by two levels over the 16-byte slots and over the 8-byte copy, the copies made, the changes of geometry by either kernel"""
    import ctypes
    import modimizer_amd as mg
    out = (ctypes.c_uint64 * 9)()
    mg.check(mg.lib().mgTableDiag(ms, out))
    return dict(zip(DIAG, (int(x) for x in out)))


SCAN_MODES = ("ANY", "POW2", "FAST", "ODD", "ODD32", "ANY32")      # MG_MODE_* of csrc/mg_scan.hip, in their numbers' order


def scan_diag():
    """mgScanDiag: launches of the scan kernel since the process started, by the instance that was chosen: {("batch", mode, where): n}
    for the batch scan (where = 1: positions / read ids asked for) and {("iter", mode): n} for the per-read iterator's kernel"""
    import ctypes
    import modimizer_amd as mg
    out = (ctypes.c_uint64 * 18)()
    mg.check(mg.lib().mgScanDiag(out))
    d = {}
    for m, name in enumerate(SCAN_MODES):
        d[("batch", name, 0)] = int(out[2 * m]); d[("batch", name, 1)] = int(out[2 * m + 1]); d[("iter", name)] = int(out[12 + m])
    return d


def scan_diag_since(before):
    """the instances launched since `before` (a scan_diag ()), with their counts: what did not run is not in it"""
    now = scan_diag()
    return {key: now[key] - before[key] for key in now if now[key] != before[key]}


XFER_DIAG = ("transfers", "pieces", "threads", "piece_bytes", "sparse_by_pagemap", "sparse_plain", "sparse_runs", "sparse_skipped")


def xfer_diag():
    """mgXferDiag: what the array transfers' team (csrc/mg_xfer.hip) has done on the current device since the process started: transfers
    run, pieces moved, threads of the last transfer, bytes per piece in force, sparse uploads by the page map and by the plain copy,
    runs of pages the last sparse upload sent and bytes it did not send"""
    import ctypes
    import modimizer_amd as mg
    out = (ctypes.c_uint64 * 8)()
    mg.lib().mgXferDiag(out)
    return dict(zip(XFER_DIAG, (int(x) for x in out)))


# ---- the probe libraries of oracle/ (prefix_probe.hip, devsort_probe.hip, xfer_probe.hip, hash_probe.hip): a hash of their sources is baked into them ----

ORACLE = os.path.join(ROOT, "oracle")


def probe_source_hash(sources):
    """the hash oracle/Makefile bakes into a probe: sha256 over the `sha256sum` listing of its sources (paths as the Makefile names them,
    relative to oracle/), 16 hex digits"""
    listing = "".join("%s  %s\n" % (hashlib.sha256(open(os.path.join(ORACLE, n), "rb").read()).hexdigest(), n) for n in sources)
    return hashlib.sha256(listing.encode()).hexdigest()[:16]


def probe_binary_hash(path, marker):
    """the hash a built probe carries behind `<marker>=`, read out of the file (no dlopen); None if there is no such file or marker"""
    try:
        m = re.search(marker.encode() + rb"=([0-9a-f]{16})", open(path, "rb").read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def build_probe(lib_name, marker, sources):
    """make oracle/<lib_name> if the one in the tree is not the build of the tree's sources (build() of the entry point makes it with
    the rest); its path"""
    path = os.path.join(ORACLE, lib_name)
    if probe_binary_hash(path, marker) != probe_source_hash(sources):
        subprocess.check_call(["make", "-C", ORACLE, "-s", lib_name])
    return path
