"""Blocked-gzip (BGZF) FASTA / FASTQ through the DEVICE text parser (mg_textgpu.hip and the mg_text*.hip files behind it, over mg_bgzfsrc.hip): the file is inflated on the
device into the window buffers, parsed by the same kernels as plain text, its record ids cut out by the id kernels, and a FASTQ file
that breaks a rule handed to the host parser at a TEXT offset.  Against the host parser on the plain text (records, ids), against the
plain file and MODGPU_BGZF_HOST=1 (modsets), against MODGPU_TEXT_HOST=1 (the hand-over).  mgTextFileDiag says which way a file went,
mgInflateDiag what was inflated and uploaded.  Small members (64, 100 bytes) put record starts, line ends and CR LF pairs on member
edges; 4 KiB windows put them on window edges that are no member edges."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import fasta
from tests import util
from tests.test_gpu_text import BROKEN, _awkward_ids, crafted_fasta, crafted_fastq, device_records, last_line_is_header
from tests.test_seqio import added_line, parse_file

pytestmark = pytest.mark.gpu

WINDOW = 4096
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- records ----

TEXTS = {
    "fa_mixed": lambda: crafted_fasta(np.random.default_rng(1), 200, "mixed"),
    "fa_tiny": lambda: crafted_fasta(np.random.default_rng(2), 3000, "tiny"),
    "fa_long": lambda: crafted_fasta(np.random.default_rng(3), 30, "long"),
    "fq_lf": lambda: crafted_fastq(np.random.default_rng(4), 1200),
    "fq_crlf": lambda: crafted_fastq(np.random.default_rng(5), 500, True),
}


def text_and_records(name, tmp_path_factory):
    """(text, the host parser's records of the plain file): made once per text"""
    def make():
        text = TEXTS[name]()
        if name.startswith("fa") and last_line_is_header(text):
            text += b"ACGT\n"
        path = str(tmp_path_factory.mktemp("bgzf_text") / ("t." + name[:2]))
        open(path, "wb").write(text)
        return text, parse_file(path, 1 << 40, 4)[1]
    return cached(("text", name), make)


@pytest.mark.parametrize("name", list(TEXTS))
@pytest.mark.parametrize("block", [64, 4096, 65280])
@pytest.mark.parametrize("window_kb,batch_bases", [(0, 0), (4, 3000), (8, 0)])
def test_bgzf_records_equal_host_parser(name, block, window_kb, batch_bases, tmp_path, tmp_path_factory):
    text, want = text_and_records(name, tmp_path_factory)
    blob = mg.bgzf_bytes(text, block=block)
    path = str(tmp_path / "t.gz")
    open(path, "wb").write(blob)
    env = {}
    if window_kb:
        env["TEXT_WINDOW_KB"] = window_kb
    if batch_bases:
        env["FILE_BATCH_BASES"] = batch_bases
    with mg.knobs(**env):
        rc, got = device_records(path)
        diag, inf = mg.text_file_diag(), mg.inflate_diag()
    assert rc == 0, mg.lib().mgLastError()
    assert diag["path"] == 2 and diag["text"] == len(text) and diag["handed_over"] == 0
    if window_kb:
        assert diag["windows"] == -(-len(text) // (window_kb << 10))
    assert inf["members"] == len(mg.bgzf_members(blob)) and inf["text"] == len(text)
    assert len(got) == len(want)
    fq = name.startswith("fq")
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a & 3, b & 3) if fq else np.array_equal(a, b), (i, len(a), len(b))


def test_plain_file_reports_path_1(tmp_path, tmp_path_factory):
    text, want = text_and_records("fa_mixed", tmp_path_factory)
    path = str(tmp_path / "t.fa")
    open(path, "wb").write(text)
    rc, got = device_records(path)
    assert rc == 0 and len(got) == len(want)
    d = mg.text_file_diag()
    assert d["path"] == 1 and d["text"] == len(text) and mg.inflate_diag()["members"] == 0
    with mg.knobs(TEXT_HOST=1):
        assert device_records(path)[0] == -2 and mg.text_file_diag()["path"] == 0


# ---- ids ----

def query_text(fmt, crlf, seed, golden_dir):
    """the queries of test_query_file_device_parser_equals_host_parser (awkward ids, wrapped FASTA / FASTQ) with four crafted ones, placed by
    padding the description of the record before: an id of 10 000 bytes without white space (more than two windows of 4 KiB), an empty id,
    an id whose last byte is a window's last byte, a record whose first byte is a window's first byte.  Returns (text, checks)"""
    rng = np.random.default_rng(seed)
    names, bases, offs = fasta.read_fasta(os.path.join(golden_dir, "ref.fa"))
    refseqs = [bases[offs[i]:offs[i + 1]] for i in range(len(names))]
    n = 260
    ids = _awkward_ids(rng, n)
    eol = b"\r\n" if crlf else b"\n"
    mark = b">" if fmt == "fa" else b"@"
    letters = np.frombuffer(b"ACGT", np.uint8)
    special = {60: "long", 61: "empty", 120: "id_ends_window", 180: "starts_window"}
    out, size, checks = [], 0, {}

    def record(core, tail, txt):
        if fmt == "fa":
            return mark + core + tail + eol + b"".join(txt[j:j + 61] + eol for j in range(0, len(txt), 61))
        return mark + core + tail + eol + txt + eol + b"+" + eol + b"I" * len(txt) + eol

    prev = None                                             # (core, tail, txt) of the record not yet written: its description may still grow
    for i, (core, tail) in enumerate(ids):
        u = rng.random()
        if u < 0.6:
            s = refseqs[int(rng.integers(0, len(refseqs)))]
            ln = int(rng.integers(30, 1500)); a = int(rng.integers(0, max(1, len(s) - ln)))
            b = s[a:a + ln].copy()
            if rng.random() < 0.5:
                b = (3 - b[::-1]).astype(np.uint8)
        else:
            b = rng.integers(0, 4, int(rng.integers(0, 400))).astype(np.uint8)
        txt = letters[b].tobytes()
        kind = special.get(i)
        if kind == "long":
            core, tail = b"L" + b"0123456789" * 1000, b""
            assert len(core) > 2 * WINDOW
        elif kind == "empty":
            core, tail = b"", b" the id is empty"
        elif kind in ("id_ends_window", "starts_window"):
            core, tail = b"placed_%d" % i, b" d"
            p_core, p_tail, p_txt = prev
            if not p_tail:
                p_tail = b" pad"
            start = size + len(record(p_core, p_tail, p_txt))                 # where this record would start
            want = (WINDOW - 1 - len(core)) if kind == "id_ends_window" else 0      # this record's first byte, modulo the window
            p_tail += b"x" * ((want - start) % WINDOW)
            prev = (p_core, p_tail, p_txt)
        if prev is not None:
            r = record(*prev); out.append(r); size += len(r)
        if kind:
            checks[kind] = (size, len(core))
        prev = (core, tail, txt)
    out.append(record(*prev))
    text = b"".join(out)
    at, ln = checks["id_ends_window"]
    assert (at + ln) % WINDOW == WINDOW - 1 and text[at:at + 1] == mark and text[at + 1 + ln:at + 2 + ln] == b" "      # the id's last byte ends a window
    at, _ = checks["starts_window"]
    assert at % WINDOW == 0 and text[at - 1:at + 1] == b"\n" + mark
    at, ln = checks["long"]
    assert text[at + 1:at + 1 + ln].isalnum() and at // WINDOW + 2 < (at + ln) // WINDOW
    at, _ = checks["empty"]
    assert text[at:at + 2] == mark + b" "
    return text, n


def run_query(qpath, golden_dir, tmp_path, **kn):
    L = mg.lib()
    with mg.knobs(**kn):
        sh = mg.seqhashCreate(15, 8, 17); ms = mg.modsetCreate(sh, 20)
        ref = L.mgReferenceCreate(ms, 1 << 26)
        out = str(tmp_path / "o.txt")
        with mg.CFile(out, "w") as f:
            assert L.mgReferenceFastaRead(ref, os.path.join(golden_dir, "ref.fa").encode(), True, f) == 0
            assert L.mgQueryFile(ref, qpath.encode(), f) == 0, L.mgLastError()
        diag = mg.text_file_diag()
        L.mgReferenceDestroy(ref); L.modsetDestroy(ms)
    return open(out, "rb").read(), diag


def query_case(fmt, crlf, golden_dir, tmp_path_factory):
    """(text, records, the plain path, the host parser's output on the plain file): once per format"""
    def make():
        text, n = query_text(fmt, crlf, 23, golden_dir)
        d = tmp_path_factory.mktemp("bgzf_query")
        plain = str(d / ("q." + fmt))
        open(plain, "wb").write(text)
        host, diag = run_query(plain, golden_dir, d, TEXT_HOST=1)
        assert diag["path"] == 0 and host.count(b"\nQ\t") >= n - 1 and host.count(b"\nM\t") > 5
        return text, n, plain, host
    return cached(("query", fmt, crlf), make)


@pytest.mark.parametrize("fmt,crlf", [("fa", False), ("fq", False), ("fa", True), ("fq", True)])
@pytest.mark.parametrize("block", [100, 65280])
@pytest.mark.parametrize("window_kb,batch_bases", [(4, 2500), (0, 0)])
def test_bgzf_query_ids_equal_host_parser(fmt, crlf, block, window_kb, batch_bases, golden_dir, tmp_path, tmp_path_factory):
    text, n, plain, host = query_case(fmt, crlf, golden_dir, tmp_path_factory)
    qpath = str(tmp_path / "q.gz")
    open(qpath, "wb").write(mg.bgzf_bytes(text, block=block))
    kn = dict(TEXT_WINDOW_KB=window_kb, FILE_BATCH_BASES=batch_bases) if window_kb else {}
    got, diag = run_query(qpath, golden_dir, tmp_path, **kn)
    assert diag["path"] == 2 and diag["text"] == len(text)
    assert got == host, [x for x in zip(got.splitlines(), host.splitlines()) if x[0] != x[1]][:3]


@pytest.mark.parametrize("fmt,crlf", [("fa", False), ("fq", False), ("fa", True), ("fq", True)])
@pytest.mark.parametrize("window_kb,batch_bases", [(4, 2500), (0, 0)])
def test_id_kernels_equal_host_team_on_plain_text(fmt, crlf, window_kb, batch_bases, golden_dir, tmp_path, tmp_path_factory):
    """the same plain file with MODGPU_TEXT_IDS_DEVICE=1 and with the knob unset: the id kernels against the host team on identical text"""
    text, n, plain, host = query_case(fmt, crlf, golden_dir, tmp_path_factory)
    kn = dict(TEXT_WINDOW_KB=window_kb, FILE_BATCH_BASES=batch_bases) if window_kb else {}
    team, d0 = run_query(plain, golden_dir, tmp_path, **kn)
    kern, d1 = run_query(plain, golden_dir, tmp_path, TEXT_IDS_DEVICE=1, **kn)
    assert d0["path"] == 1 and d1["path"] == 1
    assert kern == team == host


# ---- modsets ----

ADD_CODE = r"""
import sys, os, numpy as np
import modimizer_amd as mg
L = mg.lib()
fn = getattr(L, sys.argv[1])
for tag, path, kn in (("plain", sys.argv[2], {}), ("bgzf", sys.argv[3], {}), ("bgzf_host", sys.argv[3], dict(BGZF_HOST=1))):
    with mg.knobs(**kn):
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
def test_add_sequence_file_bgzf_vs_plain(fname, api, golden_dir, tmp_path):
    plain = os.path.join(golden_dir, fname)
    bgz = str(tmp_path / (fname + ".gz"))
    blob = mg.bgzf_bytes(open(plain, "rb").read(), block=1000)
    open(bgz, "wb").write(blob)
    r = subprocess.run([sys.executable, "-c", ADD_CODE, api, plain, bgz, str(tmp_path)], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=util.ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in r.stdout.splitlines()}
    assert rows["plain"][:2] == [1, 0] and rows["bgzf"][:2] == [2, 0] and rows["bgzf_host"][0] == 0
    assert rows["bgzf"][2] == len(blob) and rows["bgzf_host"][2] == 0      # one walk: every compressed byte uploaded once
    lines = {t: open(str(tmp_path / (t + ".txt"))).read() for t in rows}
    arrs = {t: np.load(str(tmp_path / (t + ".npy"))) for t in rows}
    for t in ("bgzf", "bgzf_host"):
        assert lines[t] == lines["plain"] and np.array_equal(arrs[t], arrs["plain"]), t
    tag = "seqio_%s.stdout.txt" % fname.replace(".", "_")
    if api == "mgAddSequenceFile" and os.path.exists(os.path.join(golden_dir, tag)):
        assert lines["bgzf"].strip() == added_line(util.golden_text(tag))


def test_one_walk_uploads_every_byte_once(golden_dir, tmp_path):
    """the parser walks a file once, so the compressed bytes pass through the source's ring: after the call as many bytes were uploaded as
    the file has -- nothing twice, nothing skipped -- over windows and members that do not align"""
    L = mg.lib()
    text = crafted_fasta(np.random.default_rng(8), 150, "mixed")
    if last_line_is_header(text):
        text += b"ACGT\n"
    blob = mg.bgzf_bytes(text, block=777)
    path = str(tmp_path / "t.fa.gz")
    open(path, "wb").write(blob)
    for kn in ({}, dict(TEXT_WINDOW_KB=4)):
        with mg.knobs(**kn):
            sh = mg.seqhashCreate(15, 4, 17); ms = mg.modsetCreate(sh, 20)
            with mg.CFile(str(tmp_path / "l.txt"), "w") as f:
                assert L.mgAddSequenceFile(ms, path.encode(), f) == 0, L.mgLastError()
            inf = mg.inflate_diag()
            L.modsetDestroy(ms)
        assert inf["uploaded"] == len(blob) and inf["text"] == len(text) and mg.text_file_diag()["path"] == 2


# ---- the hand-over ----

HAND_CODE = r"""
import sys, numpy as np
import modimizer_amd as mg
L = mg.lib()
sh = mg.seqhashCreate(15, 4, 17); ms = mg.modsetCreate(sh, 20)
with mg.CFile(sys.argv[2], "w") as f:
    rc = L.mgAddSequenceFile(ms, sys.argv[1].encode(), f)
d = mg.text_file_diag()
open(sys.argv[3], "w").write("%d %d" % (d["path"], d["handed_over"]))
mg.check(L.modsetSyncToHost(ms, 0))
v, dp, _ = mg.modset_arrays(ms)
print("rc", rc, "max", ms.contents.max, "sum", int(v[1:].sum() % (1 << 61)), int(dp[1:].astype(np.int64).sum()))
"""


def expected_hand_over(text, bad_pos, window, batch):
    """the parser's batching restated: at a window's end the accumulator holds the sequence-line bytes and the completed records since the
    last flush; it is flushed there if it holds `batch` bases and a record.  The window that holds byte bad_pos (None: the text's last
    window, where a file that ends inside a record is noticed) ends the device's part: the host parser starts after the last flush."""
    b = np.frombuffer(text, np.uint8)
    nl = b == 10
    line = np.concatenate([[0], np.cumsum(nl)[:-1]])
    base_cum = np.concatenate([[0], np.cumsum((line % 4 == 1) & ~nl)])
    rec_end = np.flatnonzero(nl & (line % 4 == 3))          # a record's last newline
    resume = 0
    for e in range(window, len(text) + window, window):
        e = min(e, len(text))
        if (bad_pos is not None and bad_pos < e) or (bad_pos is None and e == len(text)):
            return resume
        done = rec_end[(rec_end >= resume) & (rec_end < e)]
        if len(done) and base_cum[e] - base_cum[resume] >= batch:
            resume = int(done[-1]) + 1
    raise AssertionError("the text ended before the breach")


@pytest.mark.parametrize("kind", list(BROKEN))
@pytest.mark.parametrize("block", [64, 65280])
def test_bgzf_fastq_that_breaks_the_rules_goes_to_the_host_parser(kind, block, tmp_path):
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
    if kind == "no_plus":
        assert text[bad_pos:bad_pos + 1] == b"-"
    if kind == "no_at":
        assert text[bad_pos:bad_pos + 1] == b"#"
    want_off = expected_hand_over(text, bad_pos, 8192, 5000)
    assert want_off > 0 and text[want_off - 1:want_off + 1] == b"\n@"
    path = str(tmp_path / "bad.fq.gz")
    open(path, "wb").write(mg.bgzf_bytes(text, block=block))
    res, diags = [], []
    for host in ("1", "0"):
        env = dict(os.environ, MODGPU_TEXT_HOST=host, MODGPU_TEXT_WINDOW_KB="8", MODGPU_FILE_BATCH_BASES="5000", PYTHONPATH=util.ROOT)
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
        assert diags[0] == "0 0" and diags[1] == "2 %d" % want_off, (diags, want_off)


def test_hand_over_offset_of_a_fatal_breach(tmp_path):
    """the breaches the host parser dies of leave no diag behind in the test above: here the device parser alone is asked (the test hook maps the
    hand-over to -2 and adds nothing), and mgTextFileDiag names the text offset it would have handed on"""
    rng = np.random.default_rng(9)
    lines = crafted_fastq(rng, 1500).split(b"\n")[:-1]
    recs = [b"\n".join(lines[4 * i:4 * i + 4]) + b"\n" for i in range(len(lines) // 4)]
    starts = np.cumsum([0] + [len(r) for r in recs])
    recs[901] = b"#" + recs[901][1:]
    text = b"".join(recs)
    want_off = expected_hand_over(text, int(starts[901]), 8192, 5000)
    for block in (64, 65280):
        path = str(tmp_path / ("bad%d.fq.gz" % block))
        open(path, "wb").write(mg.bgzf_bytes(text, block=block))
        with mg.knobs(TEXT_WINDOW_KB=8, FILE_BATCH_BASES=5000):
            assert device_records(path)[0] == -2
            d = mg.text_file_diag()
        assert d["path"] == 2 and d["handed_over"] == want_off > 0, (d, want_off)


# ---- what the parser declines; a corrupt member ----

DECL_CODE = HAND_CODE
SPANNING = b">a\nACGTACGTACGTACGT\n>lonely " + b"x" * 150 + b"\n"      # header_last.fa's last line lies inside one member of 64 bytes: this one's spans three
assert (SPANNING.rfind(b"\n>") + 1) // 64 + 2 <= (len(SPANNING) - 1) // 64


def declined_files(golden_dir, tmp_path):
    raw = open(os.path.join(golden_dir, "mixed.fa"), "rb").read()
    out = {}
    for name, blob in (("unterminated", mg.bgzf_bytes(open(os.path.join(golden_dir, "unterminated.fa"), "rb").read(), block=1000)),
                       ("header_last", mg.bgzf_bytes(open(os.path.join(golden_dir, "header_last.fa"), "rb").read(), block=64)),
                       ("header_last_spanning", mg.bgzf_bytes(SPANNING, block=64)),
                       ("gzip_member_appended", mg.bgzf_bytes(raw[:3000], block=999, eof=False) + gzip.compress(raw[3000:6000])),
                       ("cut_in_last_block", mg.bgzf_bytes(raw, block=999, eof=False)[:-40])):
        out[name] = str(tmp_path / (name + ".gz"))
        open(out[name], "wb").write(blob)
    return out


@pytest.mark.parametrize("name", ["unterminated", "header_last", "header_last_spanning", "gzip_member_appended", "cut_in_last_block"])
def test_bgzf_the_device_parser_declines(name, golden_dir, tmp_path):
    path = declined_files(golden_dir, tmp_path)[name]
    rc, _ = device_records(path)
    assert rc == -2 and mg.text_file_diag()["path"] == 0, name
    res = []
    for host in ("0", "1"):                                 # mgAddSequenceFile: what the host reader gives, whoever inflates
        env = dict(os.environ, MODGPU_BGZF_HOST=host, PYTHONPATH=util.ROOT)
        line, dg = str(tmp_path / ("l%s.txt" % host)), str(tmp_path / ("d%s.txt" % host))
        r = subprocess.run([sys.executable, "-c", DECL_CODE, path, line, dg], capture_output=True, text=True, env=env)
        err = "\n".join(l for l in r.stderr.splitlines() if "amdgpu.ids" not in l)
        res.append((r.returncode, r.stdout, err, open(line).read() if os.path.exists(line) else "", open(dg).read() if os.path.exists(dg) else None))
    assert res[0] == res[1], res
    if res[0][4] is not None:
        assert res[0][4] == "0 0"


def test_ordinary_gzip_stays_with_the_host_parser(golden_dir):
    assert device_records(os.path.join(golden_dir, "mixed.fa.gz"))[0] == -2 and mg.text_file_diag()["path"] == 0


def test_corrupt_member_in_mid_file_fails_the_call(tmp_path):
    """one payload byte flipped in member 15 of 30: the first and the last members pass the parser's look at the text's edges, the device
    meets the bad one (by its status: the kernel writes nothing out of place) and the call fails, naming the member's file offset"""
    text = crafted_fasta(np.random.default_rng(12), 40, "mixed")
    if last_line_is_header(text):
        text += b"ACGT\n"
    block = -(-len(text) // 29)
    blob = bytearray(mg.bgzf_bytes(text, block=block, eof=True))
    members = mg.bgzf_members(bytes(blob))
    assert len(members) == 30
    pay, clen = members[15][0], members[15][1]
    blob[pay + clen // 2] ^= 0x55
    at = pay - 18                                           # the member's first byte (bgzf_bytes writes the 18-byte header)
    assert bytes(blob[at:at + 4]) == b"\x1f\x8b\x08\x04"
    path = str(tmp_path / "corrupt.fa.gz")
    open(path, "wb").write(bytes(blob))
    code = r"""
import sys
import modimizer_amd as mg
L = mg.lib()
sh = mg.seqhashCreate(15, 4, 17); ms = mg.modsetCreate(sh, 20)
with mg.CFile(sys.argv[2], "w") as f:
    rc = L.mgAddSequenceFile(ms, sys.argv[1].encode(), f)
print("rc", rc, L.mgLastError().decode(), flush=True)
sys.exit(1 if rc else 0)
"""
    r = subprocess.run([sys.executable, "-c", code, path, str(tmp_path / "l.txt")], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=util.ROOT))
    msg = r.stdout + r.stderr
    assert r.returncode != 0, msg
    assert "corrupt" in msg and "file offset %d" % at in msg, msg
