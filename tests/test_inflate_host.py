"""The raw-deflate decoder of csrc/mg_inflate_core.h, compiled for the host (mgInflateMemberHost), against Python's zlib.

The corpus below is also what tests/test_gpu_inflate.py puts through the kernel and what tools/inflate_host_check.c runs under the
sanitizers (write_corpus, tools/asan_inflate.sh).  Every member is a raw-deflate payload with the length and CRC-32 a gzip trailer would state; for a corrupt
one zlib's verdict is the yardstick: where zlib refuses (or length or CRC differ) the status is non-zero and nothing outside the output
range is written, where zlib accepts the bytes are equal."""
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

import modimizer_amd as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- text
def fastq_text(n, seed=1):
    rng = random.Random(seed)
    out = []
    size = 0
    i = 0
    while size < n:
        k = rng.randint(30, 400)
        rec = "@read%d/%d len=%d\n%s\n+\n%s\n" % (i, rng.randint(1, 2), k, "".join(rng.choice("ACGT") if rng.random() > 0.01 else "N" for _ in range(k)),
                                                "".join(chr(33 + min(60, max(0, int(rng.gauss(30, 8))))) for _ in range(k)))
        out.append(rec); size += len(rec); i += 1
    return "".join(out).encode()[:n]


def fasta_text(n, seed=2):
    rng = random.Random(seed)
    out = []
    size = 0
    i = 0
    while size < n:
        k = rng.randint(100, 9000)
        seq = "".join(rng.choice("ACGTacgt") for _ in range(k))
        rec = ">contig%d some description %d\n%s\n" % (i, k, "\n".join(seq[j:j + 60] for j in range(0, k, 60)))
        out.append(rec); size += len(rec); i += 1
    return "".join(out).encode()[:n]


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


# ---------------------------------------------------------------------------------------------------------------- a bit writer
class Bits:
    """deflate's bit order: fields from the least significant bit up, Huffman codes with their most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):
        self.acc |= value << self.n; self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xff); self.acc >>= 8; self.n -= 8

    def code(self, code, bits):
        self.put(int(format(code, "0%db" % bits)[::-1], 2), bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self, pad=0):
        self.align()
        return bytes(self.out) + b"\0" * pad

    # the fixed code (RFC 1951 3.2.6)
    def fixed_sym(self, s):
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xC0 + s - 280, 8)

    def fixed_match(self, length, dist):
        ls, lx, lv = length_code(length)
        self.fixed_sym(ls); self.put(lv, lx)
        ds, dx, dv = dist_code(dist)
        self.code(ds, 5); self.put(dv, dx)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def length_code(length):
    i = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_code(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def canonical(lens):
    """{symbol: (code, bits)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2); over-subscribed sets get codes all the same"""
    code, out = 0, {}
    for bits in range(1, 16):
        for s, b in enumerate(lens):
            if b == bits:
                out[s] = (code & ((1 << bits) - 1), bits); code += 1
        code <<= 1
    return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [2, 2, 2] + [0] * 13 + [3, 4, 4]           # the code-length code of the hand-made headers: 0, 1, 2 in two bits, 16 in three, 17 and 18 in four


def dynamic_header(w, hlit, hdist, cl_syms, final=1, cl_lens=CL_LENS):
    """a dynamic block's header: HLIT, HDIST (the fields' values), the code-length code, then cl_syms: [(symbol, extra value)]"""
    w.put(final, 1); w.put(2, 2); w.put(hlit, 5); w.put(hdist, 5); w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(cl_lens[s], 3)
    codes = canonical(cl_lens)
    for s, x in cl_syms:
        w.code(*codes[s])
        if s >= 16:
            w.put(x, {16: 2, 17: 3, 18: 7}[s])


def zeros(n):
    """n zero lengths as 18 / 17 runs and single zeros"""
    out = []
    while n >= 11:
        k = min(n, 138); out.append((18, k - 11)); n -= k
    if n >= 3:
        out.append((17, n - 3)); n = 0
    return out + [(0, 0)] * n


def hand_dynamic(lit_lens, dist_lens, body, cl_tail=None):
    """a dynamic block with these literal/length lengths {symbol: bits} (257 codes or as many as the highest symbol asks for) and distance lengths [bits]; body (w, lit codes, dist codes) writes the data"""
    w = Bits()
    syms, at = [], 0
    for s in sorted(lit_lens):
        syms += zeros(s - at) + [(lit_lens[s], 0)]; at = s + 1
    nlit = max(257, max(lit_lens) + 1)
    syms += zeros(nlit - at)
    syms += cl_tail if cl_tail is not None else [(b, 0) for b in dist_lens]
    dynamic_header(w, nlit - 257, len(dist_lens) - 1, syms)
    lens = [0] * nlit
    for s, b in lit_lens.items():
        lens[s] = b
    body(w, canonical(lens), canonical(dist_lens))
    return w.bytes()


# ---------------------------------------------------------------------------------------------------------------- the corpus
def member(name, payload, text, want=None, device=True):
    """want: statistics the member must show, {name: (op, value)}"""
    return dict(name=name, payload=bytes(payload), text=bytes(text), ulen=len(text), crc=zlib.crc32(text), want=want or {},
                device=device and len(payload) <= 65536)


_GOOD = None


def good_corpus():
    global _GOOD
    if _GOOD is not None:
        return _GOOD
    fq, fa = fastq_text(65280), fasta_text(65280)
    out = [member("empty", bytes.fromhex("0300"), b"", dict(fixed=("==", 1))),
           member("one_byte", deflate(b"A"), b"A")]
    for n in (65526, 65535, 65536):                        # (zlib ends a level-0 stream with an empty stored block) 65526: 65536 bytes of payload; 65536: both blocks hold text
        data = fq[:n] + b"x" * (n - len(fq))
        out.append(member("stored_%d" % n, deflate(data, 0), data, dict(stored=("==", 2), dynamic=("==", 0), fixed=("==", 0))))
    out.append(member("fixed_4k", deflate(fq[:4096], 6, zlib.Z_FIXED), fq[:4096], dict(fixed=(">=", 1), dynamic=("==", 0))))
    for kind, data in (("fq", fq), ("fa", fa)):
        for level, strat, sname in ((1, zlib.Z_DEFAULT_STRATEGY, "l1"), (6, zlib.Z_DEFAULT_STRATEGY, "l6"), (9, zlib.Z_DEFAULT_STRATEGY, "l9"),
                                    (6, zlib.Z_RLE, "rle"), (6, zlib.Z_HUFFMAN_ONLY, "huff")):
            out.append(member("%s_%s" % (kind, sname), deflate(data, level, strat), data, dict(dynamic=(">=", 1))))
            out.append(member("%s_%s_mem1" % (kind, sname), deflate(data, level, strat, 1), data, dict(dynamic=(">", 1))))
    out.append(member("equal_bytes", deflate(b"\x55" * 65536, 9), b"\x55" * 65536, dict(distance=("==", 1), match=("==", 258))))
    # Fibonacci frequencies under Z_HUFFMAN_ONLY: 22 literals, 46367 bytes: the rarest get the longest code deflate allows
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = bytearray(b"".join(bytes([65 + i]) * f for i, f in enumerate(fib)))
    random.Random(3).shuffle(data)
    out.append(member("fibonacci", deflate(bytes(data), 6, zlib.Z_HUFFMAN_ONLY), data, dict(litlen_bits=("==", 15))))
    # hand-assembled: the top distance and length codes (zlib itself never emits a distance above 32506)
    base = fa[:32768]
    w = Bits()
    w.put(0, 1); w.put(0, 2); w.align(); w.put(32768, 16); w.put(32768 ^ 0xffff, 16); w.out += base
    w.put(1, 1); w.put(1, 2); w.fixed_match(258, 32768); w.fixed_sym(256)
    out.append(member("dist_32768_len_258", w.bytes(), base + base[:258], dict(distance=("==", 32768), match=("==", 258), stored=("==", 1), fixed=("==", 1))))
    w = Bits()
    w.put(1, 1); w.put(1, 2)
    for ch in b"HELLO":
        w.fixed_sym(ch)
    w.fixed_match(10, 5); w.fixed_sym(256)
    out.append(member("dist_equals_produced", w.bytes(), b"HELLOHELLOHELLO", dict(distance=("==", 5))))
    # the incomplete codes zlib accepts: a single distance code of one bit; and a 16 that repeats the last literal/length length into the distance lengths
    def body(w, lit, dist):
        w.code(*lit[65]); w.code(*lit[257]); w.code(*dist[0]); w.code(*lit[256])
    out.append(member("single_distance_code", hand_dynamic({65: 1, 256: 2, 257: 2}, [1], body), b"AAAA", dict(dist_bits=("==", 1))))
    def body(w, lit, dist):
        for s in (65, 66, 65, 256):
            w.code(*lit[s])
    out.append(member("repeat_across_boundary", hand_dynamic({65: 1, 66: 2, 256: 2}, [2, 2, 2, 2], body, cl_tail=[(16, 1)]), b"ABA", dict(dist_bits=("==", 2))))
    every = b"".join(bytes([v]) * 256 for v in range(256))
    out.append(member("every_byte_stored", deflate(every, 0), every, dict(stored=("==", 2))))
    out.append(member("every_byte_dynamic", deflate(every, 6), every, dict(dynamic=(">=", 1))))
    shuffled = bytearray(every[:32768] + every[-8192:]); random.Random(4).shuffle(shuffled)
    out.append(member("every_byte_literals", deflate(bytes(shuffled), 6, zlib.Z_HUFFMAN_ONLY), shuffled, dict(dynamic=(">=", 1))))
    _GOOD = out
    return out


def corrupt(name, payload, ulen, crc, device=True):
    return dict(name=name, payload=bytes(payload), ulen=ulen, crc=crc, device=device and len(payload) <= 65536)


_BAD = None


def corrupt_corpus():
    """members that are wrong somewhere, or look it; the verdict is zlib's (zlib_verdict)"""
    global _BAD
    if _BAD is not None:
        return _BAD
    fq = fastq_text(4096, 5)
    pay = deflate(fq, 6)
    crc = zlib.crc32(fq)
    out = [corrupt("wrong_crc", pay, 4096, crc ^ 0x10), corrupt("one_short", pay, 4095, zlib.crc32(fq[:4095])), corrupt("one_long", pay, 4097, crc)]
    out.append(corrupt("block_type_3", b"\x07" + b"\0" * 8, 0, 0))
    w = Bits(); w.put(1, 1); w.put(0, 2); w.align(); w.put(4, 16); w.put(4 ^ 0xfffe, 16); w.out += b"abcd"
    out.append(corrupt("stored_nlen", w.bytes(), 4, zlib.crc32(b"abcd")))
    for hlit in (30, 31):
        w = Bits(); w.put(1, 1); w.put(2, 2); w.put(hlit, 5); w.put(0, 5); w.put(15, 4)
        out.append(corrupt("hlit_%d" % hlit, w.bytes(64), 1, 0))
    w = Bits(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(30, 5); w.put(15, 4)
    out.append(corrupt("hdist_30", w.bytes(64), 1, 0))
    def lit_only(w, lit, dist):
        w.code(*lit[65]); w.code(*lit[256])
    out.append(corrupt("oversubscribed_lengths", hand_dynamic({65: 1, 66: 1, 256: 1}, [1], lit_only) + b"\0" * 8, 1, zlib.crc32(b"A")))
    out.append(corrupt("incomplete_lengths", hand_dynamic({65: 2, 256: 2}, [1], lit_only) + b"\0" * 8, 1, zlib.crc32(b"A")))
    out.append(corrupt("incomplete_distances", hand_dynamic({65: 1, 256: 1}, [2, 2], lit_only) + b"\0" * 8, 1, zlib.crc32(b"A")))
    out.append(corrupt("no_end_of_block", hand_dynamic({65: 1, 66: 1}, [1], lambda w, lit, dist: w.code(*lit[65])) + b"\0" * 8, 1, zlib.crc32(b"A")))
    w = Bits(); dynamic_header(w, 0, 0, [(0, 0)] * 4, cl_lens=[1, 1, 1] + [0] * 16)            # the code-length code itself over-subscribed
    out.append(corrupt("oversubscribed_code_lengths", w.bytes(16), 1, 0))
    w = Bits(); dynamic_header(w, 0, 0, [(0, 0)] * 4, cl_lens=[2, 2] + [0] * 17)               # ... and incomplete
    out.append(corrupt("incomplete_code_lengths", w.bytes(16), 1, 0))
    w = Bits(); dynamic_header(w, 0, 0, [(16, 0)] + zeros(255))
    out.append(corrupt("leading_16", w.bytes(16), 1, 0))
    for s, x, n in ((16, 3, 6), (17, 7, 10), (18, 127, 138)):                                       # a run of n lengths with n - 1 places left of 258
        w = Bits(); dynamic_header(w, 0, 0, zeros(258 - n) + [(1, 0)] + [(s, x)] if s == 16 else zeros(258 - n + 1) + [(s, x)])
        out.append(corrupt("run_%d_overruns" % s, w.bytes(16), 1, 0))
    for s in (286, 287):
        w = Bits(); w.put(1, 1); w.put(1, 2); w.fixed_sym(65); w.fixed_sym(s); w.put(0, 5); w.fixed_sym(256)
        out.append(corrupt("fixed_symbol_%d" % s, w.bytes(8), 4, 0))
    for d in (30, 31):
        w = Bits(); w.put(1, 1); w.put(1, 2); w.fixed_sym(65); w.fixed_sym(257); w.code(d, 5); w.fixed_sym(256)
        out.append(corrupt("distance_code_%d" % d, w.bytes(8), 4, 0))
    w = Bits(); w.put(1, 1); w.put(1, 2); w.fixed_sym(65); w.fixed_match(3, 2); w.fixed_sym(256)
    out.append(corrupt("distance_past_start", w.bytes(), 4, 0))
    for k in range(1, 9):
        out.append(corrupt("cut_%d" % k, pay[:-k], 4096, crc))
    rng = random.Random(6)
    for i in range(256):
        at = rng.randrange(len(pay))
        flipped = bytearray(pay); flipped[at] ^= 1 << rng.randrange(8)
        out.append(corrupt("flip_%03d_at_%d" % (i, at), flipped, 4096, crc))
    _BAD = out
    return out


def zlib_verdict(m):
    """the text if zlib inflates the payload to the end of its last block and length and CRC-32 are as stated, else None"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(m["payload"], m["ulen"] + 1)
    except zlib.error:
        return None
    if not d.eof or len(text) != m["ulen"] or zlib.crc32(text) != m["crc"]:
        return None
    return text


def write_corpus(path):
    """the corpus as tools/inflate_host_check.c reads it: a count, then per member cLen, uLen, crc (little-endian words) and the payload"""
    ms = good_corpus() + corrupt_corpus()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(ms)))
        for m in ms:
            f.write(struct.pack("<III", len(m["payload"]), m["ulen"], m["crc"]) + m["payload"])
    return ms


# ---------------------------------------------------------------------------------------------------------------- tests
OPS = {"==": lambda a, b: a == b, ">=": lambda a, b: a >= b, ">": lambda a, b: a > b}


@pytest.mark.parametrize("m", good_corpus(), ids=lambda m: m["name"])
def test_good_member_inflates_to_zlibs_bytes(m):
    assert zlib_verdict(m) == m["text"], "the corpus itself: zlib does not accept this member"
    status, text, stats, intact = mg.inflate_member_host(m["payload"], m["ulen"], m["crc"])
    assert status == 0, mg.INFLATE_STATUS[status]
    assert text == m["text"] and intact
    for key, (op, value) in m["want"].items():
        assert OPS[op](stats[key], value), "the corpus does not reach what it claims: %s is %d, not %s %d (%r)" % (key, stats[key], op, value, stats)


def test_corpus_reaches_every_block_type_and_the_long_codes():
    tot = {}
    for m in good_corpus():
        stats = mg.inflate_member_host(m["payload"], m["ulen"], m["crc"])[2]
        for k, v in stats.items():
            tot[k] = max(tot.get(k, 0), v)
    assert tot["stored"] >= 2 and tot["fixed"] >= 1 and tot["dynamic"] > 1
    assert tot["litlen_bits"] == 15 and tot["distance"] == 32768 and tot["match"] == 258


@pytest.mark.parametrize("m", corrupt_corpus()[:-256], ids=lambda m: m["name"])
def test_corrupt_member_gets_zlibs_verdict(m):
    check_against_zlib(m)


def test_single_byte_flips_get_zlibs_verdict():
    accepted = 0
    for m in corrupt_corpus()[-256:]:
        accepted += check_against_zlib(m)
    assert accepted < 256


def check_against_zlib(m):
    want = zlib_verdict(m)
    status, text, _, intact = mg.inflate_member_host(m["payload"], m["ulen"], m["crc"])
    assert intact, "%s: bytes outside the output range were written" % m["name"]
    if want is None:
        assert status != 0, "%s: zlib refuses this member" % m["name"]
        return 0
    assert status == 0 and text == want, "%s: zlib accepts this member (%s)" % (m["name"], mg.INFLATE_STATUS[status])
    return 1


EXPECTED_STATUS = dict(wrong_crc=8, one_short=7, one_long=7, block_type_3=2, stored_nlen=3, hlit_30=4, hlit_31=4, hdist_30=4, oversubscribed_lengths=4,
                       incomplete_lengths=4, incomplete_distances=4, no_end_of_block=4, oversubscribed_code_lengths=4, incomplete_code_lengths=4, leading_16=4,
                       run_16_overruns=4, run_17_overruns=4, run_18_overruns=4, fixed_symbol_286=5, fixed_symbol_287=5, distance_code_30=5, distance_code_31=5,
                       distance_past_start=6, cut_8=1)


def test_each_refusal_has_its_own_status():
    by_name = {m["name"]: m for m in corrupt_corpus()}
    for name, want in EXPECTED_STATUS.items():
        m = by_name[name]
        assert zlib_verdict(m) is None, name
        status = mg.inflate_member_host(m["payload"], m["ulen"], m["crc"])[0]
        assert status == want, "%s: %s, not %s" % (name, mg.INFLATE_STATUS[status], mg.INFLATE_STATUS[want])


def test_crc_slices_equal_zlib_at_every_small_length():
    """the CRC is computed in 64 slices joined by the CRC's linearity: every length below 200, and lengths around the slices' edges"""
    rng = random.Random(7)
    data = bytes(rng.randrange(256) for _ in range(65536))
    for n in list(range(200)) + [4095, 4096, 4097, 65471, 65472, 65473, 65535, 65536]:
        pay = deflate(data[:n], 0)
        assert mg.inflate_member_host(pay, n, zlib.crc32(data[:n]))[0] == 0, n
        assert mg.inflate_member_host(pay, n, zlib.crc32(data[:n]) ^ 1)[0] == 8, n


def test_guard_page_program_agrees_over_the_corpus(tmp_path):
    """tools/inflate_host_check.c: the decoder alone, in a process of its own, every member between inaccessible pages that end (then begin) exactly at
    its two ranges.  Its statuses are the library's.  (tools/asan_inflate.sh builds the same program with the sanitizers, on the build host.)"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe, corpus = str(tmp_path / "inflate_host_check"), str(tmp_path / "corpus.bin")
    build = subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "modimizer_amd", "csrc"),
                            os.path.join(ROOT, "tools", "inflate_host_check.c"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    ms = write_corpus(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("member") and "status" in ln]
    assert len(lines) == len(ms)
    for ln, m in zip(lines, ms):
        assert int(ln[3]) == mg.inflate_member_host(m["payload"], m["ulen"], m["crc"])[0], m["name"]
