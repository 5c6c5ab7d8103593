"""Blocked gzip (BGZF) inflated on the device: the kernel (mg_inflate.hip) against the decoder's host compile, which test_inflate_host.py
holds against zlib; then the files -- mgCompositionFile and mgSeqConvertFile on BGZF versions of their goldens against the same calls on
the plain files, the knob, the files that must keep today's path, a corrupt member, and mgBgzfInflateFile against zlib."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import modimizer_amd as mg
from tests import test_composition as tc
from tests import test_inflate_host as th
from tests import test_seqconvert as ts
from tests import util

pytestmark = pytest.mark.gpu

GUARD = 0xA5
MG_ERR_ARG = 3


# ---------------------------------------------------------------------------------------------------------------- the kernel
def lay_out(ms, gap=3, lead=0, trail=0):
    """members packed into one compressed and one text buffer, `gap` bytes between neighbours (odd: the offsets turn odd), `lead` / `trail`
    bytes before the first and after the last: (comp bytes, table, out bytes)"""
    comp, table, u = bytearray(b"\xee" * lead), [], lead
    for m in ms:
        table.append((len(comp), len(m["payload"]), u, m["ulen"], m["crc"]))
        comp += m["payload"] + b"\xee" * gap
        u += m["ulen"] + gap
    if ms:
        del comp[len(comp) - gap:]
        u -= gap
    return bytes(comp) + b"\xee" * trail, table, u + trail


_HOST = {}


def host_result(m):
    """(status, text) of the host compile, computed once per member"""
    if m["name"] not in _HOST:
        _HOST[m["name"]] = mg.inflate_member_host(m["payload"], m["ulen"], m["crc"])[:2]
    return _HOST[m["name"]]


def run_and_check(ms, **layout):
    comp, table, out_bytes = lay_out(ms, **layout)
    out, status, n_bad = mg.inflate_members_device(comp, table, out_bytes, GUARD)
    covered = np.zeros(out_bytes, bool)
    want_bad = 0
    for m, (c_off, c_len, u_off, u_len, crc), st in zip(ms, table, status):
        want_st, want_text = host_result(m)
        assert int(st) == want_st, (m["name"], mg.INFLATE_STATUS[int(st)], mg.INFLATE_STATUS[want_st])
        if not want_st:
            assert out[u_off:u_off + u_len].tobytes() == want_text, m["name"]
        want_bad += want_st != 0
        covered[u_off:u_off + u_len] = True
    assert n_bad == want_bad
    assert (out[~covered] == GUARD).all(), "a byte between the members' output ranges was written"
    d = mg.inflate_diag()
    assert d["members"] == len(ms) and d["launches"] == 1 and d["text"] == sum(m["ulen"] for m in ms)
    return status


def device_corpus():
    return [m for m in th.good_corpus() + th.corrupt_corpus() if m["device"]]


def test_corpus_good_and_corrupt_in_one_launch():
    """every member of the host test's corpus that a BGZF member can be (65536 bytes at most, compressed and not), good and corrupt mixed, odd
    offsets, the first member at byte 0 of both buffers and the last ending at their last byte: statuses and bytes are the host compile's,
    nBad counts the bad ones, the gaps keep their guard bytes"""
    ms = device_corpus()
    assert sum(1 for m in ms if host_result(m)[0]) > 200 and sum(1 for m in ms if not host_result(m)[0]) > 25
    assert {"stored_65526", "fibonacci", "dist_32768_len_258", "equal_bytes", "fq_l6_mem1", "empty"} <= {m["name"] for m in ms}
    status = run_and_check(ms)
    assert set(int(s) for s in status) >= {0, 1, 2, 3, 4, 5, 6, 7, 8}


SMALL = ["empty", "one_byte", "fixed_4k", "dist_equals_produced", "single_distance_code", "repeat_across_boundary", "wrong_crc", "block_type_3", "cut_3",
         "distance_past_start", "one_long"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_launch_sizes(n):
    by_name = {m["name"]: m for m in device_corpus()}
    ms = [by_name[SMALL[(i * 7 + n) % len(SMALL)]] for i in range(n)]
    run_and_check(ms, gap=1 + n % 2 * 2, lead=n % 3, trail=n % 2)


def test_a_full_member_at_both_ends_of_both_buffers():
    by_name = {m["name"]: m for m in device_corpus()}
    for name in ("stored_65526", "equal_bytes"):
        run_and_check([by_name[name]], gap=0)
        run_and_check([by_name[name], by_name[name]], gap=0)


def test_refused_before_a_launch():
    m = next(m for m in device_corpus() if m["name"] == "fixed_4k")
    pay, n = m["payload"], len(m["payload"])
    big = pay + b"\0" * (65537 - n)
    cases = [(big, [(0, 65537, 0, m["ulen"], m["crc"])], 70000),                       # cLen = 65537
             (pay, [(0, n, 0, 65537, m["crc"])], 70000),                               # uLen = 65537
             (pay, [(1, n, 0, m["ulen"], m["crc"])], 70000),                           # the payload leaves its buffer
             (pay, [(0, n, 1, m["ulen"], m["crc"])], m["ulen"]),                       # the text leaves its buffer
             (pay, [(0, n, 0, m["ulen"], m["crc"]), (2 ** 40, n, 0, m["ulen"], m["crc"])], 70000)]
    for comp, table, out_bytes in cases:
        with pytest.raises(mg.ModgpuError) as e:
            mg.inflate_members_device(comp, table, out_bytes, GUARD)
        assert e.value.status == MG_ERR_ARG
        assert mg.inflate_diag() == dict(members=0, uploaded=0, text=0, launches=0)
    out, status, n_bad = mg.inflate_members_device(pay, [(0, n, 0, m["ulen"], m["crc"])], m["ulen"], GUARD)      # the bounds themselves are fine
    assert n_bad == 0 and out.tobytes() == m["text"]


# ---------------------------------------------------------------------------------------------------------------- files
ALL_COMP = mg.COMP_BASES | mg.COMP_QUALS | mg.COMP_LENGTHS
BLOCKS = [65280, 999, 37]
WINDOWS = [None, 4]


def comp_call(path, flags=ALL_COMP):
    out, err, res = mg.composition_file(path, flags)
    return out, err, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in res.items()}


def members_of(blob):
    """file offsets of the members of a BGZF blob"""
    at, out = 0, []
    while at < len(blob):
        out.append(at)
        at += int.from_bytes(blob[at + 16:at + 18], "little") + 1
    return out


_PLAIN = {}


def plain_composition(name, kb):
    if (name, kb) not in _PLAIN:
        with mg.knobs(TEXT_WINDOW_KB=kb):
            _PLAIN[name, kb] = comp_call(os.path.join(tc.GOLDEN, name))
    return _PLAIN[name, kb]


@pytest.mark.parametrize("kb", WINDOWS)
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", ["comp_long.fa", "comp_many.fq"])
def test_composition_of_a_bgzf_file(name, block, kb, tmp_path):
    raw = open(os.path.join(tc.GOLDEN, name), "rb").read()
    blob = mg.bgzf_bytes(raw, block)
    path = str(tmp_path / (name + ".gz"))
    open(path, "wb").write(blob)
    with mg.knobs(TEXT_WINDOW_KB=kb):
        got = comp_call(path)
        d, cd = mg.inflate_diag(), mg.composition_diag()
    assert got == plain_composition(name, kb)
    n_text = (len(raw) + block - 1) // block
    assert n_text <= d["members"] <= n_text + 1 and d["text"] == len(raw) and d["launches"] >= 1, d
    assert 0 < d["uploaded"] <= len(blob), (d, len(blob))
    if kb:
        assert cd["windows"] == (len(raw) + 4095) // 4096


@pytest.mark.parametrize("stem,path,runs", ts.goldens(), ids=[g[0] for g in ts.goldens()])
def test_seqconvert_of_a_bgzf_file(stem, path, runs, tmp_path):
    """every recorded mode of every golden: the call on the BGZF file does what the call on the plain file does -- output, stderr, counters, or
    the refusal and no file.  The block size goes round 65280, 999, 37 with the goldens, the window is one tile for every other one"""
    raw = open(path, "rb").read()
    k = [g[0] for g in ts.goldens()].index(stem)
    block, kb = BLOCKS[k % 3], WINDOWS[(k // 3) % 2]
    blob = mg.bgzf_bytes(raw, block)
    bz = str(tmp_path / "in.gz")
    open(bz, "wb").write(blob)
    with mg.knobs(TEXT_WINDOW_KB=kb):
        for mode in runs:
            outs = []
            for src in (path, bz):
                dst = str(tmp_path / ("out_%s_%d" % (mode, len(outs))))
                try:
                    err, res = mg.seq_convert_file(src, dst, ts.MODES[mode])
                    outs.append((open(dst, "rb").read(), err, res))
                except mg.ModgpuError as e:
                    assert not os.path.exists(dst)
                    outs.append(str(e).replace(src, "FILE"))
                if src == bz and raw:
                    d = mg.inflate_diag()
                    assert d["members"] >= 1 and 0 < d["uploaded"] <= len(blob), (stem, mode, d, len(blob))
            assert outs[0] == outs[1], (stem, mode, block, kb)


@pytest.mark.parametrize("name", ["comp_long.fa", "comp_many.fq"])
def test_the_knob_sends_a_bgzf_file_to_the_host(name, tmp_path):
    raw = open(os.path.join(tc.GOLDEN, name), "rb").read()
    path = str(tmp_path / (name + ".gz"))
    open(path, "wb").write(mg.bgzf_bytes(raw, 999))
    with mg.knobs(BGZF_HOST=1):
        assert comp_call(path) == plain_composition(name, None)
        assert mg.inflate_diag()["members"] == 0
        dst = str(tmp_path / "o.fa")
        err, res = mg.seq_convert_file(path, dst, mg.SEQ_FASTA)
        assert mg.inflate_diag() == dict(members=0, uploaded=0, text=0, launches=0)
    want = str(tmp_path / "want.fa")
    assert (err, res) == mg.seq_convert_file(os.path.join(tc.GOLDEN, name), want, mg.SEQ_FASTA)
    assert open(dst, "rb").read() == open(want, "rb").read()
    assert mg.inflate_diag()["members"] == 0


def test_files_that_keep_the_host_path(tmp_path):
    """BGZF followed by an ordinary gzip member, ordinary gzip, a truncated last block: equal output, nothing on the device"""
    name = "comp_many.fq"
    raw = open(os.path.join(tc.GOLDEN, name), "rb").read()
    half = len(raw) // 2
    blobs = dict(mixed=mg.bgzf_bytes(raw[:half], 999, eof=False) + gzip.compress(raw[half:]),
                 plain_gzip=gzip.compress(raw),
                 bgzf_then_junk_header=mg.bgzf_bytes(raw, 999, eof=False) + gzip.compress(b""))
    for what, blob in blobs.items():
        path = str(tmp_path / (what + ".gz"))
        open(path, "wb").write(blob)
        assert comp_call(path) == plain_composition(name, None), what
        assert mg.inflate_diag()["members"] == 0, what
    # a truncated last block is not a BGZF file from end to end: whatever today's path makes of it, the device is not asked
    path = str(tmp_path / "cut.gz")
    open(path, "wb").write(mg.bgzf_bytes(raw, 999)[:-40])
    try:
        comp_call(path)
    except mg.ModgpuError:
        pass
    assert mg.inflate_diag()["members"] == 0


@pytest.mark.parametrize("kb", WINDOWS)
@pytest.mark.parametrize("name", ["comp_cut_seq.fq", "comp_cut_qual.fq", "comp_cut_hdr.fq", "comp_hdr_nonl.fa", "comp_hdr_end.fa"])
def test_an_unfinished_last_record(name, kb, tmp_path):
    """the record is dropped with the program's message and the text is walked again up to the cut: as on the plain file"""
    src = os.path.join(tc.GOLDEN, name)
    raw = open(src, "rb").read()
    path = str(tmp_path / (name + ".gz"))
    open(path, "wb").write(mg.bgzf_bytes(raw, 37))
    with mg.knobs(TEXT_WINDOW_KB=kb):
        want = comp_call(src)
        got = comp_call(path)
        d = mg.inflate_diag()
        assert got == want and "incomplete sequence record" in want[1]
        assert d["members"] >= 1 and d["uploaded"] <= os.path.getsize(path)
        a, b = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
        assert mg.seq_convert_file(src, a, mg.SEQ_FASTA) == mg.seq_convert_file(path, b, mg.SEQ_FASTA)
        assert open(a, "rb").read() == open(b, "rb").read()


def test_a_byte_flipped_mid_file(tmp_path):
    raw = open(os.path.join(tc.GOLDEN, "comp_many.fq"), "rb").read()
    blob = bytearray(mg.bgzf_bytes(raw, 999))
    starts = members_of(bytes(blob))
    at = starts[len(starts) // 2]
    blob[at + 18 + 40] ^= 0x04                            # inside the deflate payload of a member in the middle
    path = str(tmp_path / "flipped.fq.gz")
    open(path, "wb").write(blob)
    for kb in WINDOWS:
        with mg.knobs(TEXT_WINDOW_KB=kb):
            with pytest.raises(mg.ModgpuError) as e:
                mg.composition_file(path, ALL_COMP)
            assert path in str(e.value) and "offset %d " % at in str(e.value), str(e.value)
            assert e.value.out == b""
            dst = str(tmp_path / "o.fq")
            with pytest.raises(mg.ModgpuError) as e:
                mg.seq_convert_file(path, dst, mg.SEQ_FASTQ)
            assert path in str(e.value) and "offset %d " % at in str(e.value), str(e.value)
            assert not os.path.exists(dst) or os.path.getsize(dst) == 0


def test_bgzf_inflate_file(tmp_path):
    rng = np.random.default_rng(11)
    lines = rng.choice(np.frombuffer(b"ACGTacgtN!5I~", np.uint8), (30000, 101))
    lines[:, 100] = 10
    lines[::4, 0] = ord("@")
    raw = lines.tobytes()                                  # 3 MB
    blob = mg.bgzf_bytes(raw)
    src, dst = str(tmp_path / "reads.gz"), str(tmp_path / "reads.txt")
    open(src, "wb").write(blob)
    assert mg.bgzf_inflate_file(src, dst) is True
    assert open(dst, "rb").read() == gzip.decompress(blob) == raw
    d = mg.inflate_diag()
    n_text = (len(raw) + 65279) // 65280                   # (the empty end marker is a member too, if the launch reaches it)
    assert n_text <= d["members"] <= n_text + 1 and d["text"] == len(raw) and d["uploaded"] <= len(blob)
    with mg.knobs(TEXT_WINDOW_KB=4):                       # a member spans sixteen windows
        small = str(tmp_path / "small.gz")
        open(small, "wb").write(mg.bgzf_bytes(raw[:200000]))
        assert mg.bgzf_inflate_file(small, dst) is True
        assert open(dst, "rb").read() == raw[:200000]
    # not BGZF from end to end: -2, nothing written
    os.remove(dst)
    plain, ordinary = str(tmp_path / "plain.txt"), str(tmp_path / "ordinary.gz")
    open(plain, "wb").write(raw[:5000]); open(ordinary, "wb").write(gzip.compress(raw[:5000]))
    assert mg.bgzf_inflate_file(plain, dst) is False and mg.bgzf_inflate_file(ordinary, dst) is False
    assert not os.path.exists(dst)
    # examples/inflate_file.c
    libdir = os.path.join(util.ROOT, "modimizer_amd")
    exe = str(tmp_path / "inflate_file")
    r = subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c99", "-I", os.path.join(util.ROOT, "include"), os.path.join(util.ROOT, "examples", "inflate_file.c"),
                        "-o", exe, "-L", libdir, "-lmodgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(dst, "rb").read() == raw
    r = subprocess.run([exe, plain, dst], capture_output=True, text=True)
    assert r.returncode == 3 and "not a BGZF file" in r.stderr
