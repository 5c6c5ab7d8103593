"""The C-ABI boundary: libmodgpu.so loads, exports every symbol include/modgpu.h and modgpu_compat.h declare, keeps the
reference's struct layouts, and fails loudly (no CPU fallback) when there is no HIP device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import modimizer_amd as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "modgpu.h")).read() + open(os.path.join(ROOT, "include", "modgpu_compat.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set()
    for m in re.finditer(r"^[A-Za-z_][\w \t\*]*?[\s\*]([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", src, flags=re.M):
        names.add(m.group(1))
    return names


def test_library_exports_every_declared_symbol():
    L = mg.lib()
    decl = header_functions()
    assert len(decl) > 50
    missing = [n for n in sorted(decl) if not hasattr(L, n)]
    assert not missing, missing
    assert set(mg.EXPORTS) <= decl | {"seqhash"}
    # and the python binding lists them all
    assert decl <= set(mg.EXPORTS), sorted(decl - set(mg.EXPORTS))


def test_struct_layouts_match_reference():
    # seqhash.h:15-23 is 80 bytes with mask at 16 and factor1 at 32 (measured on the reference)
    assert C.sizeof(mg.Seqhash) == 80
    assert mg.Seqhash.mask.offset == 16 and mg.Seqhash.shift1.offset == 24
    assert mg.Seqhash.factor1.offset == 32 and mg.Seqhash.patternRC.offset == 48
    assert C.sizeof(mg.SeqhashRCiterator) == 72
    assert mg.SeqhashRCiterator.hashBuf.offset == 40 and mg.SeqhashRCiterator.isDone.offset == 68
    assert mg.Modset.index.offset == 32 and mg.Modset.max.offset == 64 and C.sizeof(mg.Modset) == 72


def test_product_never_touches_the_oracle():
    """modimizer_amd/ (python + C/HIP sources) must not import, link or call anything under oracle/"""
    pkg = os.path.join(ROOT, "modimizer_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip", ".cpp", "Makefile")):
                txt = open(os.path.join(d, f)).read()
                assert "oracle" not in txt.lower() or f == "__init__.py" and "oracle" not in txt, (d, f)
    out = subprocess.run(["ldd", mg.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in out and "modref" not in out


no_gpu = pytest.mark.skipif(mg.lib().mgDeviceCount() > 0, reason="checks the no-device behaviour")


@no_gpu
def test_batch_path_fails_loudly_without_device():
    L = mg.lib()
    sh = mg.seqhashCreate(21, 64, 17)
    bases = np.zeros(100, np.uint8)
    offs = np.array([0, 100], np.int64)
    with pytest.raises(mg.ModgpuError, match="no HIP device"):
        mg.scan_batch(sh, bases, offs)
    ms = mg.modsetCreate(sh, 20)
    assert L.modsetAddBatchDevice(ms, None, 10, None, 1, None) == 1      # MG_ERR_NO_DEVICE
    assert b"no CPU fallback" in L.mgLastError()
    assert L.mgAddSequenceBatch(ms, bases.ctypes.data, offs.ctypes.data, 1) == -1
    p = C.c_void_p()
    assert L.mgDeviceAlloc(C.byref(p), 64) == 1
    L.modsetDestroy(ms)


@no_gpu
@pytest.mark.parametrize("n", [100, 10000])
def test_iterator_dies_without_device(n):
    """modRCiterator needs a HIP device whichever leg a read's length selects (the scalar loop below the launch-latency
    crossover, one kernel launch above it): with no device it die()s like every reference error (utils.c:19-30)"""
    code = ("import numpy as np, modimizer_amd as mg\n"
            "sh = mg.seqhashCreate(21, 64, 17)\n"
            "mg.iterate(sh, np.zeros(%d, np.uint8))\n" % n)
    env = dict(os.environ, MODGPU_NO_TORCH="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "FATAL ERROR" in r.stderr and "modRCiterator" in r.stderr and "no HIP device" in r.stderr


def test_binary_carries_the_hash_of_its_sources(tmp_path, monkeypatch):
    """libmodgpu.so is git-ignored yet rides along to the GPU box, so the binary says what it was built from --
    csrc/Makefile bakes a hash of every source into it (mg_version.c), the binding recomputes it from the tree, and a library whose
    hash differs is rebuilt before it is loaded (modimizer_amd.build); smoke() asserts equality."""
    import shutil
    L = mg.lib()
    h = mg.source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    assert L.mgSourceHash().decode() == h == mg.binary_hash()
    assert L.mgVersion().decode().endswith("src=" + h)
    # any change to any source changes the tree's hash: the unchanged binary is then seen as stale
    csrc = tmp_path / "csrc"
    shutil.copytree(mg.CSRC, csrc, ignore=shutil.ignore_patterns("*.o"))
    monkeypatch.setattr(mg, "CSRC", str(csrc))
    assert mg.source_hash() == h
    for name in ("mg_scan.hip", "mg_host.c", "mg_common.h", "Makefile"):
        p = os.path.join(str(csrc), name)
        old = open(p, "rb").read()
        open(p, "ab").write(b"\n")
        assert mg.source_hash() != h, name
        open(p, "wb").write(old)
        assert mg.source_hash() == h
    # a library file without the marker (or none at all) has no hash
    assert mg.binary_hash(str(tmp_path / "nothing.so")) is None


def block_uses():
    """every mgBlockReduce / mgBlockInclusive / mgBlockExclusive<THREADS, Op> the library's kernels call, THREADS as a number: a macro is
    resolved through the #define of its file or of mg_prefix.h (MG_GROUP_THREADS), one macro may name another"""
    csrc = mg.CSRC
    define = re.compile(r"^#define[ \t]+(\w+)[ \t]+(\w+)", re.M)
    common = dict(define.findall(open(os.path.join(csrc, "mg_prefix.h")).read()))
    uses = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip"):
            continue
        src = open(os.path.join(csrc, f)).read()
        macros = dict(common, **dict(define.findall(src)))
        for m in re.finditer(r"\bmgBlock(Reduce|Inclusive|Exclusive)\s*<\s*(\w+)\s*,\s*(\w+)\s*>", src):
            t = m.group(2)
            for _ in range(8):
                if t.isdigit():
                    break
                assert t in macros, (f, m.group(0), "what is %s?" % t)
                t = macros[t]
            assert t.isdigit(), (f, m.group(0))
            uses.append((f, m.group(1), int(t), m.group(3)))
    return uses


def test_probe_covers_every_block_instantiation_of_the_library():
    """what the library instantiates of mg_prefix.h's workgroup primitives is what tests/test_gpu_prefix.py drives through the probe: a
    kernel that starts to call, say, mgBlockExclusive<512, MgMax> fails here until the probe and its table cover that pair"""
    import test_gpu_prefix as tp
    uses = block_uses()
    assert len(uses) >= 20 and {u[1] for u in uses} == {"Reduce", "Inclusive", "Exclusive"}      # the regex still finds them
    assert ("mg_settext.hip", "Reduce", 1024, "MgMax") in uses                                      # ST_SCAN_THREADS -> MG_GROUP_THREADS -> 1024
    pairs = tp.block_pairs()
    missing = sorted({u for u in uses if (u[2], u[3]) not in pairs})
    assert not missing, missing
    # and the probe's source instantiates what the table lists
    src = open(os.path.join(ROOT, "oracle", "prefix_probe.hip")).read()
    for t, op, bits in tp.BLOCK_INSTANTIATIONS:
        assert re.search(r"case %d:" % t, src) and "probeBlockThreads<%s, U%d>" % (tp.OPS[op], bits) in src, (t, op, bits)


def test_probe_carries_the_hash_of_its_sources():
    """libprefixprobe.so is git-ignored and rides along like libmodgpu.so: oracle/Makefile bakes a hash of prefix_probe.hip and
    mg_prefix.h into it, the tests recompute it from the tree, and a probe of other sources is rebuilt before it is used"""
    import test_gpu_prefix as tp
    h = tp.probe_source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    tp.build_probe()
    assert tp.probe_binary_hash() == h
    assert tp.probe_binary_hash(os.path.join(ROOT, "oracle", "no_such.so")) is None


def test_devsort_tiles_are_the_headers():
    """MG_SCAN_TILE and MG_RSORT_TILE as tests/test_gpu_devsort.py states them (and the other test files take them from there) are
    mg_devsort.h's: a tile that changes moves every edge those tests are built around"""
    import test_gpu_devsort as td
    header = dict(re.findall(r"^#define[ \t]+(MG_\w+_TILE)[ \t]+(\d+)\b", open(os.path.join(mg.CSRC, "mg_devsort.h")).read(), re.M))
    assert header == {"MG_SCAN_TILE": str(td.MG_SCAN_TILE), "MG_RSORT_TILE": str(td.MG_RSORT_TILE)}
    assert td.WAVE_PART * 4 == td.MG_RSORT_TILE and td.WAVE_PART % 64 == 0      # mg_devsort.hip: four waves a tile, 64 elements a round


def test_devsort_probe_carries_the_hash_of_its_sources():
    """libdevsortprobe.so rides along like libprefixprobe.so: a hash of devsort_probe.hip, mg_devsort.h and mg_common.h is baked into it,
    the tests recompute it from the tree, and a probe of other sources is rebuilt before it is used"""
    import test_gpu_devsort as td
    h = td.probe_source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    td.build_probe()
    assert td.probe_binary_hash() == h
    assert td.probe_binary_hash(os.path.join(ROOT, "oracle", "no_such.so")) is None


def test_xfer_probe_carries_the_hash_of_its_sources():
    """libxferprobe.so rides along like the other two probes: a hash of xfer_probe.hip, mg_xfer.h and mg_common.h is baked into it, the
    tests recompute it from the tree, and a probe of other sources is rebuilt before it is used"""
    import test_gpu_xfer as tx
    h = tx.probe_source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    tx.build_probe()
    assert tx.probe_binary_hash() == h
    assert tx.probe_binary_hash(os.path.join(ROOT, "oracle", "no_such.so")) is None
    assert tx.probe().xferProbeHash().decode() == h


def test_hash_probe_carries_the_hash_of_its_sources():
    """libhashprobe.so rides along like the other three probes: a hash of hash_probe.hip and mg_common.h is baked into it, the tests
    recompute it from the tree, and a probe of other sources is rebuilt before it is used"""
    import test_gpu_hashprobe as th
    h = th.probe_source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    th.build_probe()
    assert th.probe_binary_hash() == h
    assert th.probe_binary_hash(os.path.join(ROOT, "oracle", "no_such.so")) is None
    assert th.probe().hashProbeHash().decode() == h


def test_scan_census_is_bound_and_counts_nothing_without_a_scan():
    import util
    d = util.scan_diag()
    assert len(d) == 18 and {key[1] for key in d} == set(util.SCAN_MODES)
    assert d == util.scan_diag() and util.scan_diag_since(d) == {}
    # the names the tests give the counters are mg_scan.hip's mode numbers, in order
    modes = dict(re.findall(r"^#define[ \t]+MG_MODE_(\w+)[ \t]+(\d+)\b", open(os.path.join(mg.CSRC, "mg_scan.hip")).read(), re.M))
    assert modes.pop("COUNT") == "6" and modes == {name: str(i) for i, name in enumerate(util.SCAN_MODES)}


def test_xfer_census_is_bound_and_counts_nothing_without_a_transfer():
    import util
    d = util.xfer_diag()
    assert tuple(d) == util.XFER_DIAG and len(d) == 8
    assert d == util.xfer_diag()


def test_reading_an_untouched_page_makes_it_exist():
    """what mgXferH2DSparse is for, and what tests/test_gpu_xfer.py holds it to, shown without a device: the pages of a fresh anonymous
    mapping do not exist (xferProbePresentPages, from /proc/self/pagemap); a write makes the page written exist; a plain copy OUT of the
    range, which only reads, makes every page of it exist"""
    import test_gpu_xfer as tx
    X = tx.probe()
    n = 64 * tx.PAGE + 100
    base = X.xferProbeMapAnon(n)
    assert base
    try:
        bitmap, count = tx.present_pages(X, base, n)
        if bitmap is None:
            print("/proc/self/pagemap cannot be read here")
            return
        assert count == 0 and len(bitmap) == 65
        host = tx.mapped(base, n)
        host[5 * tx.PAGE + 1] = 7
        bitmap, count = tx.present_pages(X, base, n)
        assert bitmap[5] == 1 and 1 <= count < 65           # (one page where the kernel maps 4 KiB pages on a write, more with huge pages)
        bitmap, _ = tx.present_pages(X, base + 16, n - 16)
        assert len(bitmap) == 65 and bitmap[5] == 1
        bitmap, _ = tx.present_pages(X, base + 6 * tx.PAGE, tx.PAGE)
        assert len(bitmap) == 1
        copy = host.copy()
        assert copy[5 * tx.PAGE + 1] == 7 and int(copy.sum()) == 7
        bitmap, count = tx.present_pages(X, base, n)
        assert count == 65 and np.all(bitmap == 1)
    finally:
        X.xferProbeUnmap(base, n)
