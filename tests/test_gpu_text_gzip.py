"""Ordinary gzip FASTA / FASTQ through the DEVICE text parser (mg_textgpu.hip over mg_gzipsrc.hip and mg_gunzip.hip): the file is inflated on the
device chunk by chunk into the window buffers and parsed by the kernels of plain text; its compressed bytes pass through a bounded range (one walk).
The text's size and end are not known before the last batch: the loop ends on the source's word, and a FASTA text that ends unfinished is handed to
the host parser at its last record.  Against the host parser on the plain text (records, ids), against the plain file and MODGPU_GZIP_HOST=1
(modsets), against MODGPU_TEXT_HOST=1 (the hand-overs).  Every case sets GZIP_MIN_KB=0: the files are far below the default threshold."""
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests.test_gpu_gunzip import ALL_COMP, comp_call, ran_on_device
from tests.test_gpu_text import BROKEN, crafted_fasta, crafted_fastq, device_records, last_line_is_header
from tests.test_gpu_text_bgzf import (HAND_CODE, SPANNING, TEXTS, expected_hand_over, query_case, run_query, text_and_records)
from tests.test_seqio import parse_file

pytestmark = pytest.mark.gpu

WINDOW = 4096
GZIP_KNOBS = [(4, 3), (32, 64)]                             # (GZIP_CHUNK_KB, GZIP_BATCH)
WALK = dict(GZIP_MIN_KB=0, GZIP_CHUNK_KB=4, GZIP_BATCH=3, FILE_PIECE_KB=4)


def same_records(got, want, fq):
    return len(got) == len(want) and all(np.array_equal(a & 3, b & 3) if fq else np.array_equal(a, b) for a, b in zip(got, want))


def host_records(text, path):
    open(path, "wb").write(text)
    return parse_file(path, 1 << 40, 4)[1]


def check_whole(path, text, want, fq, **kn):
    """the file through the test hook: every record, path 3, the whole text parsed on the device, nothing handed over"""
    with mg.knobs(GZIP_MIN_KB=0, **kn):
        rc, got = device_records(path)
        diag = mg.text_file_diag()
    assert rc == 0, mg.lib().mgLastError()
    assert diag["path"] == 3 and diag["text"] == len(text) and diag["handed_over"] == 0, diag
    if kn.get("TEXT_WINDOW_KB"):
        assert diag["windows"] == -(-len(text) // (kn["TEXT_WINDOW_KB"] << 10))
    assert same_records(got, want, fq)
    return diag


# ---- records ----

@pytest.mark.parametrize("name", list(TEXTS))
@pytest.mark.parametrize("level", [1, 6, 0])
@pytest.mark.parametrize("chunk_kb,batch", GZIP_KNOBS)
@pytest.mark.parametrize("window_kb,batch_bases", [(0, 0), (4, 3000), (8, 0)])
def test_gzip_records_equal_host_parser(name, level, chunk_kb, batch, window_kb, batch_bases, tmp_path, tmp_path_factory):
    text, want = text_and_records(name, tmp_path_factory)
    path = str(tmp_path / "t.gz")
    open(path, "wb").write(gzip.compress(text, level))
    kn = dict(GZIP_CHUNK_KB=chunk_kb, GZIP_BATCH=batch)
    if window_kb:
        kn["TEXT_WINDOW_KB"] = window_kb
    if batch_bases:
        kn["FILE_BATCH_BASES"] = batch_bases
    check_whole(path, text, want, name.startswith("fq"), **kn)


def sized(kind, size):
    """a crafted text of exactly `size` bytes: records are dropped from the end and the first header's description is padded"""
    text = crafted_fasta(np.random.default_rng(21), 12, "mixed") if kind == "fa" else crafted_fastq(np.random.default_rng(22), 80)
    mark = b"\n>" if kind == "fa" else b"\n@read"
    while len(text) > size - 20:
        text = text[:text.rfind(mark) + 1]
    if kind == "fa" and last_line_is_header(text):
        text = text[:text[:-1].rfind(b"\n>") + 1]
    eol = text.index(b"\n")
    text = text[:eol] + b" " + b"p" * (size - len(text) - 1) + text[eol:]
    assert len(text) == size and text.endswith(b"\n")
    return text


@pytest.mark.parametrize("kind", ["fa", "fq"])
@pytest.mark.parametrize("size", [3 * WINDOW, 3 * WINDOW + 1, WINDOW - 700])
def test_text_lengths_at_the_windows_edge(kind, size, tmp_path):
    """an exact multiple of the window (the source's look ahead says that no text follows), one byte more, less than one window"""
    text = sized(kind, size)
    want = host_records(text, str(tmp_path / ("t." + kind)))
    path = str(tmp_path / "t.gz")
    open(path, "wb").write(gzip.compress(text, 6))
    for chunk_kb, batch in GZIP_KNOBS:
        check_whole(path, text, want, kind == "fq", TEXT_WINDOW_KB=4, GZIP_CHUNK_KB=chunk_kb, GZIP_BATCH=batch)


# ---- members ----

def cut_in(text, what):
    """an offset in the middle of a sequence line / of a header line near the text's middle"""
    half = len(text) // 2
    start = text.index(b"\n>", half) + 1
    if what == "header":
        return start + 5
    eol = text.index(b"\n", start)
    while text[eol + 1:eol + 2] in (b">", b"\n") or text.index(b"\n", eol + 1) - eol < 10:
        eol = text.index(b"\n", eol + 1)
    return eol + 5


def members_blob(text, how):
    a, b = cut_in(text, "line"), cut_in(text, "header")
    a, b = min(a, b), max(a, b)
    assert 0 < a < b < len(text)
    if how == "two_line":
        return gzip.compress(text[:cut_in(text, "line")], 6) + gzip.compress(text[cut_in(text, "line"):], 1)
    if how == "two_header":
        return gzip.compress(text[:cut_in(text, "header")], 6) + gzip.compress(text[cut_in(text, "header"):], 6)
    if how == "three":
        return gzip.compress(text[:a], 1) + gzip.compress(text[a:b], 0) + gzip.compress(text[b:], 6)
    if how == "empty_between":
        return gzip.compress(text[:a], 6) + gzip.compress(b"") + gzip.compress(text[a:], 6)
    if how == "empty_first":
        return gzip.compress(b"") + gzip.compress(text, 6)
    assert how == "name_and_extra"                          # FEXTRA with a subfield that is not 'BC', FNAME
    body = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = body.compress(text) + body.flush()
    extra = b"XY\x04\x00abcd"
    head = b"\x1f\x8b\x08" + bytes([4 | 8]) + b"\0\0\0\0\0\xff" + len(extra).to_bytes(2, "little") + extra + b"reads.fa\0"
    return head + raw + (zlib.crc32(text) & 0xffffffff).to_bytes(4, "little") + (len(text) & 0xffffffff).to_bytes(4, "little")


@pytest.mark.parametrize("how", ["two_line", "two_header", "three", "empty_between", "empty_first", "name_and_extra"])
def test_gzip_members(how, tmp_path, tmp_path_factory):
    text, want = text_and_records("fa_mixed", tmp_path_factory)
    blob = members_blob(text, how)
    assert gzip.decompress(blob) == text
    path = str(tmp_path / "t.gz")
    open(path, "wb").write(blob)
    for chunk_kb, batch in GZIP_KNOBS:
        check_whole(path, text, want, False, TEXT_WINDOW_KB=4, FILE_BATCH_BASES=3000, GZIP_CHUNK_KB=chunk_kb, GZIP_BATCH=batch)
        assert mg.gunzip_diag()["members"] == {"two_line": 2, "two_header": 2, "three": 3, "empty_between": 3, "empty_first": 2, "name_and_extra": 1}[how]


# ---- ids ----

@pytest.mark.parametrize("fmt,crlf", [("fa", False), ("fq", False), ("fa", True), ("fq", True)])
@pytest.mark.parametrize("window_kb,batch_bases", [(4, 2500), (0, 0)])
def test_gzip_query_ids_equal_host_parser(fmt, crlf, window_kb, batch_bases, golden_dir, tmp_path, tmp_path_factory):
    text, n, plain, host = query_case(fmt, crlf, golden_dir, tmp_path_factory)
    qpath = str(tmp_path / "q.gz")
    open(qpath, "wb").write(gzip.compress(text, 6))
    kn = dict(TEXT_WINDOW_KB=window_kb, FILE_BATCH_BASES=batch_bases) if window_kb else {}
    got, diag = run_query(qpath, golden_dir, tmp_path, GZIP_MIN_KB=0, **kn)
    assert diag["path"] == 3 and diag["text"] == len(text) and diag["handed_over"] == 0
    assert got == host, [x for x in zip(got.splitlines(), host.splitlines()) if x[0] != x[1]][:3]


# ---- modsets ----

ADD_CODE = r"""
import sys, os, numpy as np
import modimizer_amd as mg
L = mg.lib()
fn = getattr(L, sys.argv[1])
for tag, path, kn in (("plain", sys.argv[2], {}), ("gzip", sys.argv[3], {}), ("gzip_host", sys.argv[3], dict(GZIP_HOST=1))):
    with mg.knobs(GZIP_MIN_KB=0, **kn):
        sh = mg.seqhashCreate(15, 4, 17); ms = mg.modsetCreate(sh, 20)
        with mg.CFile(os.path.join(sys.argv[4], tag + ".txt"), "w") as f:
            assert fn(ms, path.encode(), f) == 0, L.mgLastError()
        d, inf = mg.text_file_diag(), mg.inflate_diag()
        mg.check(L.modsetSyncToHost(ms, 0))
        v, dp, _ = mg.modset_arrays(ms)
        np.save(os.path.join(sys.argv[4], tag + ".npy"), np.concatenate([v[1:], dp[1:].astype(np.uint64)]))
        print(tag, d["path"], d["handed_over"], inf["uploaded"], flush=True)
        L.modsetDestroy(ms)
"""


@pytest.mark.parametrize("fname", ["mixed.fa", "many.fa", "reads.fa", "mixed.fq"])
@pytest.mark.parametrize("api", ["mgAddSequenceFile", "mgAddSequenceFile10x"])
def test_add_sequence_file_gzip_vs_plain(fname, api, golden_dir, tmp_path):
    plain = os.path.join(golden_dir, fname)
    gz = str(tmp_path / (fname + ".gz"))
    blob = gzip.compress(open(plain, "rb").read(), 6)
    open(gz, "wb").write(blob)
    r = subprocess.run([sys.executable, "-c", ADD_CODE, api, plain, gz, str(tmp_path)], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=util.ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in r.stdout.splitlines()}
    assert rows["plain"][:2] == [1, 0] and rows["gzip"][:2] == [3, 0] and rows["gzip_host"][0] == 0, rows
    assert rows["gzip"][2] == len(blob) and rows["gzip_host"][2] == 0      # one walk: every compressed byte uploaded once
    lines = {t: open(str(tmp_path / (t + ".txt"))).read() for t in rows}
    arrs = {t: np.load(str(tmp_path / (t + ".npy"))) for t in rows}
    for t in ("gzip", "gzip_host"):
        assert lines[t] == lines["plain"] and np.array_equal(arrs[t], arrs["plain"]), t


# ---- one walk ----

def small_blocks(text):
    """a gzip file of deflate blocks of a few hundred bytes (memLevel 3: 512 symbols a block), so that every batch finds a block boundary in its range"""
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 3)
    return c.compress(text) + c.flush()


def walk_once(path, text, want, fq):
    with mg.knobs(**WALK):
        diag = check_whole(path, text, want, fq, **{k: v for k, v in WALK.items() if k != "GZIP_MIN_KB"})
        return mg.gzip_src_diag(), mg.inflate_diag(), diag


def test_one_walk_keeps_a_bounded_range(tmp_path):
    """the compressed bytes pass through the range: every byte uploaded once, never more of them resident than the bound, which the file exceeds four times"""
    text = crafted_fasta(np.random.default_rng(31), 420, "mixed")
    if last_line_is_header(text):
        text += b"ACGT\n"
    want = host_records(text, str(tmp_path / "t.fa"))
    blob = small_blocks(text)
    path = str(tmp_path / "t.fa.gz")
    open(path, "wb").write(blob)
    g, inf, _ = walk_once(path, text, want, False)
    assert g["bound"] == 2 * ((3 + 1) * 4096 + 4096)       # twice (chunks a batch + 1) chunks and a piece: nothing of the file's size in it
    assert len(blob) >= 4 * g["bound"], (len(blob), g)
    assert g["uploaded"] == len(blob) == inf["uploaded"] and g["peak"] <= g["bound"] and g["refills"] >= 3, g


@pytest.mark.parametrize("kind", ["stored", "repeated_line"])
def test_one_walk_range_grows_for_a_long_block(kind, tmp_path):
    """stored blocks of 65 535 bytes do not fit the first range; a text of one repeated line makes blocks of megabytes of text: the range may grow, the
    file still passes through once and never lies on the device whole"""
    if kind == "stored":
        text = crafted_fasta(np.random.default_rng(32), 200, "mixed")
        if last_line_is_header(text):
            text += b"ACGT\n"
        blob = gzip.compress(text, 0)
    else:
        text = b">one\n" + b"ACGTTGCAAGCTTCGATTAGGCATCGATCGGATTACAGGCATTCAGGCTAGCTAGGACTTAC\n" * 750000
        blob = gzip.compress(text, 6)
    want = host_records(text, str(tmp_path / "t.fa"))
    path = str(tmp_path / "t.fa.gz")
    open(path, "wb").write(blob)
    g, inf, _ = walk_once(path, text, want, False)
    assert len(blob) > g["bound"], (len(blob), g)
    assert g["uploaded"] == len(blob) == inf["uploaded"] and g["peak"] < len(blob), (g, len(blob))


# ---- FASTA that ends unfinished ----

def fasta_ends(golden_dir):
    return {"unterminated": open(os.path.join(golden_dir, "unterminated.fa"), "rb").read(),
            "header_last": open(os.path.join(golden_dir, "header_last.fa"), "rb").read(),
            "header_last_short": SPANNING,
            "header_last_spanning": b">a\n" + b"ACGTACGTACGTACGT\n" * 240 + b">lonely " + b"x" * 300 + b"\n",
            "one_record": b">only one\nACGTACGTAC\nGGTTAACC"}


def last_start(text):
    return text.rfind(b"\n>") + 1


@pytest.mark.parametrize("name", ["unterminated", "header_last", "header_last_short", "header_last_spanning", "one_record"])
def test_gzip_fasta_that_ends_unfinished_goes_to_the_host_parser(name, golden_dir, tmp_path):
    """no newline at the text's end, a header as the last line: the device parser cannot know before it gets there.  It hands on the records before the
    last one and the host parser takes the file up at the last record's '>', with its line number: the same messages, line and set as the host parser alone"""
    text = fasta_ends(golden_dir)[name]
    at = last_start(text)
    if name == "header_last_spanning":                      # the last line starts in one window of 4 KiB and ends in the next
        assert at // WINDOW < (len(text) - 1) // WINDOW and at > 0
    path = str(tmp_path / (name + ".fa.gz"))
    open(path, "wb").write(gzip.compress(text, 6))
    res, diags = [], []
    for host in ("1", "0"):
        env = dict(os.environ, MODGPU_TEXT_HOST=host, MODGPU_GZIP_MIN_KB="0", MODGPU_TEXT_WINDOW_KB="4", MODGPU_FILE_BATCH_BASES="3000", PYTHONPATH=util.ROOT)
        line, dg = str(tmp_path / ("l%s.txt" % host)), str(tmp_path / ("d%s.txt" % host))
        r = subprocess.run([sys.executable, "-c", HAND_CODE, path, line, dg], capture_output=True, text=True, env=env)
        err = "\n".join(l for l in r.stderr.splitlines() if "amdgpu.ids" not in l)
        res.append((r.returncode, r.stdout, err, open(line).read() if os.path.exists(line) else ""))
        diags.append(open(dg).read() if os.path.exists(dg) else None)
    assert res[0] == res[1], res
    assert res[0][0] == 0 and "incomplete sequence record" in res[0][2], res[0]
    assert diags[0] == "0 0" and diags[1] == "3 %d" % at, (diags, at)
    with mg.knobs(GZIP_MIN_KB=0, TEXT_WINDOW_KB=4, FILE_BATCH_BASES=3000):      # the test hook alone: nothing is returned, the diag names the offset
        assert device_records(path)[0] == -2
        d = mg.text_file_diag()
    assert d["path"] == 3 and d["handed_over"] == at and d["text"] == len(text), d


def test_a_long_last_header_is_not_judged(tmp_path):
    """the rule of the sized sources, kept: a last line that is a header of 4096 bytes or more is no id line the device parser judges -- it is a record without bases"""
    text = b">a\nACGT\n>" + b"h" * 5000 + b"\n"
    plain, path = str(tmp_path / "t.fa"), str(tmp_path / "t.fa.gz")
    open(plain, "wb").write(text); open(path, "wb").write(gzip.compress(text))
    with mg.knobs(GZIP_MIN_KB=0, TEXT_WINDOW_KB=4):
        rc_plain, got_plain = device_records(plain)
        assert rc_plain == 0 and mg.text_file_diag()["path"] == 1
        rc, got = device_records(path)
        assert rc == 0 and mg.text_file_diag()["path"] == 3
    assert same_records(got, got_plain, False) and len(got) == 2


# ---- FASTQ that breaks a rule ----

@pytest.mark.parametrize("kind", list(BROKEN))
def test_gzip_fastq_that_breaks_the_rules_goes_to_the_host_parser(kind, tmp_path):
    rng = np.random.default_rng(9)
    lines = crafted_fastq(rng, 1500).split(b"\n")[:-1]
    recs = [b"\n".join(lines[4 * i:4 * i + 4]) + b"\n" for i in range(len(lines) // 4)]
    for r in (650, 700, 901, 1200):
        recs[r] = b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % r
    starts = np.cumsum([0] + [len(r) for r in recs])
    broken = BROKEN[kind](recs)
    text = b"".join(broken)
    bad_pos = {"no_plus": int(starts[700]) + recs[700].index(b"\n+") + 1, "no_at": int(starts[901]),
               "short_qual": int(starts[650]) + len(broken[650]) - 1, "truncated": None, "three_lines_more": None}[kind]
    want_off = expected_hand_over(text, bad_pos, 8192, 5000)
    assert want_off > 0 and text[want_off - 1:want_off + 1] == b"\n@"
    path = str(tmp_path / "bad.fq.gz")
    open(path, "wb").write(gzip.compress(text, 6))
    res, diags = [], []
    for host in ("1", "0"):
        env = dict(os.environ, MODGPU_TEXT_HOST=host, MODGPU_GZIP_MIN_KB="0", MODGPU_TEXT_WINDOW_KB="8", MODGPU_FILE_BATCH_BASES="5000", PYTHONPATH=util.ROOT)
        line, dg = str(tmp_path / ("l%s.txt" % host)), str(tmp_path / ("d%s.txt" % host))
        r = subprocess.run([sys.executable, "-c", HAND_CODE, path, line, dg], capture_output=True, text=True, env=env)
        err = "\n".join(l for l in r.stderr.splitlines() if "amdgpu.ids" not in l)
        res.append((r.returncode, r.stdout, err, open(line).read() if os.path.exists(line) else ""))
        diags.append(open(dg).read() if os.path.exists(dg) else None)
    assert res[0] == res[1], res
    if kind in ("no_plus", "no_at", "short_qual"):
        assert res[0][0] != 0 and "FATAL ERROR" in res[0][2] and "line" in res[0][2]      # (the process dies inside the call: no diag file)
    else:
        assert res[0][0] == 0 and "incomplete sequence record" in res[0][2]
        assert diags[0] == "0 0" and diags[1] == "3 %d" % want_off, (diags, want_off)
    with mg.knobs(GZIP_MIN_KB=0, TEXT_WINDOW_KB=8, FILE_BATCH_BASES=5000):      # the hand-over's offset, also where the host parser dies of the breach
        assert device_records(path)[0] == -2
        d = mg.text_file_diag()
    assert d["path"] == 3 and d["handed_over"] == want_off, (d, want_off)


# ---- what the parser declines; a corrupt stream; the other callers ----

def test_gzip_the_device_parser_declines(tmp_path, tmp_path_factory):
    text, want = text_and_records("fa_mixed", tmp_path_factory)
    path = str(tmp_path / "t.fa.gz")
    open(path, "wb").write(gzip.compress(text, 6))
    for kn in (dict(GZIP_MIN_KB=0, GZIP_HOST=1), dict(GZIP_MIN_KB=0, TEXT_HOST=1), {}):      # (no knob: the file is below the default threshold)
        with mg.knobs(**kn):
            assert device_records(path)[0] == -2 and mg.text_file_diag()["path"] == 0, kn
    check_whole(path, text, want, False)
    other = str(tmp_path / "other.gz")
    open(other, "wb").write(gzip.compress(b"#" + text[1:], 6))      # neither '>' nor '@' first: known before anything is handed on
    with mg.knobs(GZIP_MIN_KB=0):
        assert device_records(other)[0] == -2 and mg.text_file_diag()["path"] == 0 and mg.gzip_src_diag()["uploaded"] == 0


def test_corrupt_stream_in_mid_file_fails_the_call(tmp_path):
    """one byte flipped in the middle of the file: the decoder meets it by its status (it writes nothing out of place, tests/test_gpu_gunzip.py), the
    call fails with the stream's file offset, and the next call of the same process works"""
    text = crafted_fasta(np.random.default_rng(12), 330, "mixed")
    if last_line_is_header(text):
        text += b"ACGT\n"
    blob = bytearray(gzip.compress(text, 6))
    assert len(blob) > 150000
    blob[len(blob) // 2] ^= 0x55
    bad, good = str(tmp_path / "corrupt.fa.gz"), str(tmp_path / "good.fa.gz")
    open(bad, "wb").write(bytes(blob)); open(good, "wb").write(gzip.compress(text, 6))
    code = r"""
import sys
import modimizer_amd as mg
L = mg.lib()
for path in sys.argv[1:3]:
    sh = mg.seqhashCreate(15, 4, 17); ms = mg.modsetCreate(sh, 20)
    with mg.CFile(sys.argv[3], "w") as f:
        rc = L.mgAddSequenceFile(ms, path.encode(), f)
    print("rc", rc, mg.text_file_diag()["path"], L.mgLastError().decode() if rc else "", flush=True)
"""
    env = dict(os.environ, MODGPU_GZIP_MIN_KB="0", MODGPU_GZIP_CHUNK_KB="4", PYTHONPATH=util.ROOT)
    r = subprocess.run([sys.executable, "-c", code, bad, good, str(tmp_path / "l.txt")], capture_output=True, text=True, env=env)
    rows = r.stdout.splitlines()
    assert r.returncode == 0 and len(rows) == 2, r.stdout + r.stderr
    assert not rows[0].startswith("rc 0") and "corrupt gzip stream at file offset" in rows[0], rows
    assert rows[1].startswith("rc 0 3"), rows


def test_the_other_callers_keep_the_resident_source(tmp_path):
    """composition may walk twice: after a parser call on the same file it still uploads the whole file once, keeps it, and counts what mgGunzipHost counts"""
    plain = os.path.join(util.ROOT, "tests", "golden", "comp_long.fa")
    raw = open(plain, "rb").read()
    path = str(tmp_path / "c.fa.gz")
    blob = gzip.compress(raw)
    open(path, "wb").write(blob)
    with mg.knobs(GZIP_MIN_KB=0, GZIP_CHUNK_KB=4, GZIP_BATCH=64, GZIP_RATIO=64):
        rc, _ = device_records(path)
        assert rc in (0, -2) and mg.text_file_diag()["path"] == 3
        want = comp_call(plain)
        walked = mg.gzip_src_diag()
        got = comp_call(path)
        d, inf = mg.gunzip_diag(), mg.inflate_diag()
        assert got == want and ran_on_device(d)
        assert inf["uploaded"] == len(blob) and mg.gzip_src_diag() == walked      # (no one-walk source was opened)
        status, text, hd, _ = mg.gunzip_host(blob, 4096, 64, 4096 * 64, len(raw))
        assert status == 0 and text == raw
        assert d == hd, (d, hd)


REF_CODE = r"""
import sys
import modimizer_amd as mg
L = mg.lib()
sh = mg.seqhashCreate(15, 8, 17); ms = mg.modsetCreate(sh, 20)
ref = L.mgReferenceCreate(ms, 1 << 26)
with mg.CFile(sys.argv[3], "w") as f:
    rc = L.mgReferenceFastaRead(ref, sys.argv[1].encode(), True, f)
    d = mg.text_file_diag()
    rq = L.mgQueryFile(ref, sys.argv[2].encode(), f)
print("rc", rc, rq, "path", d["path"], d["handed_over"], flush=True)
"""


def test_reference_file_that_ends_unfinished(golden_dir, tmp_path):
    """mgReferenceFastaRead takes the hand-over too: the records before the last go in on the device, the host parser says what the reference says about
    the last one, and the Reference answers queries as the one read by the host parser alone"""
    text = open(os.path.join(golden_dir, "ref.fa"), "rb").read().rstrip(b"\n")
    at = last_start(text)
    assert at > 0
    path = str(tmp_path / "ref.fa.gz")
    open(path, "wb").write(gzip.compress(text, 6))
    res = []
    for host in ("1", "0"):
        env = dict(os.environ, MODGPU_TEXT_HOST=host, MODGPU_GZIP_MIN_KB="0", MODGPU_TEXT_WINDOW_KB="4", MODGPU_FILE_BATCH_BASES="3000", PYTHONPATH=util.ROOT)
        out = str(tmp_path / ("o%s.txt" % host))
        r = subprocess.run([sys.executable, "-c", REF_CODE, path, os.path.join(golden_dir, "mixed.fa"), out], capture_output=True, text=True, env=env)
        err = "\n".join(l for l in r.stderr.splitlines() if "amdgpu.ids" not in l)
        res.append((r.returncode, r.stdout.replace("path 3 %d" % at, "path 0 0"), err, open(out).read() if os.path.exists(out) else ""))
        assert ("path 3 %d" % at if host == "0" else "path 0 0") in r.stdout, (host, r.stdout, err)
    assert res[0] == res[1], res
    assert res[0][0] == 0 and "rc 0 0" in res[0][1] and "incomplete sequence record" in res[0][2], res[0]
