"""modasm -o1 / -o2 / -b / -c (findOverlaps, modasm.c:314-418; markBadReads, 1266-1322; markContained, 1370-1394): a plain Python
restatement -- the pure record per pair of reads, then the replay that reads and writes the reads' `bad` flags in command order -- against the
reference program's own output for every recorded command sequence (tests/golden/ovl_*: make_golden_overlap.py), which the randomized GPU
tests (test_gpu_readset_overlap.py) then lean on; the library's host loops against the same lines and files; the flags through a file; the
lists of MgOverlaps; the error cases; the new names in header, library and binding."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import modimizer_amd as mg
from tests import util
from tests import test_readset as trs

TAGS = {"k19d8": (19, 8)}
TOPMASK, TOPBIT = 0x7fffffff, 0x80000000
BAD_REPEAT, BAD_ORDER10, BAD_ORDER1, BAD_NOMATCH, BAD_LOWHIT, BAD_LOWCOPY1 = 1, 2, 4, 8, 16, 32      # modasm.c:38-45
F_PLUS, F_CONTAINED, F_SKIPPED = 1, 2, 4
NAMES = ["mgReadsetFindOverlaps", "mgReadsetOverlapStats", "mgReadsetMarkBadReads", "mgReadsetMarkContained", "mgReadsetOverlapsPath"]
VOID_NAMES = ["mgOverlapsFree", "mgReadsetOverlapsDiag"]


# ---- the restatement: a = test_readset.lib_arrays (reads from 0 there: read i of the reference is row i - 1), info = ms's array ----

class Restatement:
    def __init__(self, a, info, bad=None, contained=None):
        self.a, self.info = a, info
        self.n = len(a["nHit"])
        self.hs = [int(v) for v in a["hitStart"]]                   # hits of read i: [hs[i - 1], hs[i])
        self.hit = [int(v) for v in a["hit"]]
        self.pos = []                                               # per hit the inclusive sum of its read's dx: xPos[j + 1], yPos at hit j
        dx = [int(v) for v in a["dx"]]
        for i in range(self.n):
            run = 0
            for h in range(self.hs[i], self.hs[i + 1]):
                run += dx[h]
                self.pos.append(run)
        self.inv_start, self.inv = [int(v) for v in a["invStart"]], [int(v) for v in a["invSpace"]]
        self.bad = [0] * (self.n + 1) if bad is None else list(bad)
        self.contained = [0] * (self.n + 1) if contained is None else list(contained)
        self.out = []
        self._pure = {}
        self.cands = {}                                             # per query looked at: the entries of the inverse lists it walks
        self.runs = {}

    # -- pure: depends on the hit lists and info / depth only --
    def pure(self, x):
        """(nRepeat, [record per pair with nHit >= 3, by nHit descending then arrival]); a record is a dict.  self.runs[x] = {y: candidates of
        (x, y)} for every y walked, the dropped ones (fewer than 3) too"""
        if x in self._pure:
            return self._pure[x]
        a0 = self.hs[x - 1]
        hx = self.hit[a0:self.hs[x]]
        hmap, n_repeat, n_hit, first, ordinal = {}, 0, {}, {}, 0
        for j, h in enumerate(hx):
            m = h & TOPMASK
            if (int(self.info[m]) & 3) != 1:
                continue
            if m in hmap:
                n_repeat += 1
                continue
            hmap[m] = j + 1
            for y in self.inv[self.inv_start[m]:self.inv_start[m + 1]]:
                if y not in n_hit:
                    n_hit[y], first[y] = 0, ordinal
                n_hit[y] += 1
                ordinal += 1
        recs = []
        for y in sorted((y for y in n_hit if n_hit[y] >= 3), key=lambda y: (-n_hit[y], first[y])):
            b0 = self.hs[y - 1]
            at = [j for j, h in enumerate(self.hit[b0:self.hs[y]]) if (h & TOPMASK) in hmap]
            match = [(hmap[self.hit[b0 + j] & TOPMASK], self.hit[b0 + j], self.pos[b0 + j]) for j in at]
            n_plus = sum(1 for ihx, h, _ in match if (h & TOPBIT) == (hx[ihx - 1] & TOPBIT))
            n_minus = len(match) - n_plus
            r = dict(iy=y, nHit=n_hit[y], isPlus=0, isContained=0, nBadOrder=0, nBadFlip=0)
            # for the tests that design a pair: the matches as (j in y, ihx in x), and the counts before either branch adjusts them
            r["match"], r["rawPlus"], r["rawMinus"] = [(j, m[0]) for j, m in zip(at, match)], n_plus, n_minus
            x_len, y_len = int(self.a["len"][x - 1]), int(self.a["len"][y - 1])
            if n_plus > n_minus:
                r["isPlus"], r["nBadFlip"] = 1, n_minus
                last = 0
                for ihx, _, y_pos in match:
                    last_diff = self.pos[a0 + ihx - 1] - y_pos
                    if not last and last_diff < 0:
                        r["isContained"] = 1
                    if ihx < last:
                        r["nBadOrder"] += 1
                        n_plus -= 1
                    last = ihx
                if r["isContained"] and x_len - last_diff > y_len:
                    r["isContained"] = 0
            elif n_minus and not n_plus:
                last = len(hx)
                for ihx, _, _ in match:
                    if ihx > last:
                        r["nBadOrder"] += 1
                        n_minus -= 1
                    last = ihx
            r["nPlus"], r["nMinus"] = n_plus, n_minus
            recs.append(r)
        self._pure[x] = (n_repeat, recs)
        self.cands[x] = ordinal
        self.runs[x] = n_hit
        self.table_size = getattr(self, 'table_size', {}); self.table_size[x] = len(hmap)
        return self._pure[x]

    # -- the replay: reads and writes bad[] in processing order --
    def find_overlaps(self, x, level):
        """the list as -b / -c see it: (iy, nHit, nBadOrder, nBadFlip, flags) per entry"""
        n_repeat, recs = self.pure(x)
        if n_repeat:
            self.bad[x] |= BAD_REPEAT
        n_good = n_bad = 0
        seen = []
        for r in recs:
            if self.bad[r["iy"]]:
                seen.append((r["iy"], r["nHit"], 0, 0, F_SKIPPED))
                continue
            is_bad = bool(r["nBadOrder"] or r["nBadFlip"])
            n_bad += is_bad
            n_good += not is_bad
            if level > 1:
                self.out.append("RH\t%u\tlen %d\t%s\t+ %d\t- %d\tbadOrder %d\t%s\n" % (
                    r["iy"], self.a["len"][r["iy"] - 1], "BAD" if is_bad else "GOOD", r["nPlus"], r["nMinus"], r["nBadOrder"],
                    "CONTAINED" if r["isContained"] else "OVERLAP"))
            seen.append((r["iy"], r["nHit"], r["nBadOrder"], r["nBadFlip"], r["isPlus"] * F_PLUS + r["isContained"] * F_CONTAINED))
        if not n_good and not n_bad:
            self.bad[x] |= BAD_NOMATCH
            if self.a["nHit"][x - 1] < 10:
                self.bad[x] |= BAD_LOWHIT
            elif self.a["nCopy"][x - 1][1] < 10:
                self.bad[x] |= BAD_LOWCOPY1
        if level > 0:
            nc = self.a["nCopy"][x - 1]
            self.out.append("RR %6u\tlen %d\tnHit %3d\tnMiss %3d\tnCpy %d %d %d %d\tnRepeatMod %d\tnGood %4d\tnBad %4d\n" % (
                x, self.a["len"][x - 1], self.a["nHit"][x - 1], self.a["nMiss"][x - 1], nc[0], nc[1], nc[2], nc[3], n_repeat, n_good, n_bad))
        return seen

    def overlap_stats(self, d):
        for x in range(d, self.n + 1, d):
            self.find_overlaps(x, 1)

    def mark_bad_reads(self):
        n = self.n
        self.bad = [0] * (n + 1)
        bad_list, n_bad, l_bad = [[] for _ in range(n + 1)], [0] * (n + 1), [0] * (n + 1)
        for x in range(1, n + 1):
            for iy, _, n_order, n_flip, _ in self.find_overlaps(x, 0):
                if n_flip or n_order:
                    n_bad[iy] += 1
                    if n_bad[iy] < 10 and l_bad[x] < 10:
                        bad_list[x].append(iy); l_bad[x] += 1
        def prune():
            for x in range(1, n + 1):
                i = l_bad[x]
                while i:
                    i -= 1
                    if self.bad[bad_list[x][i]]:
                        l_bad[x] -= 1
                        bad_list[x][i] = bad_list[x][l_bad[x]]
        count = 0
        for x in range(1, n + 1):
            if n_bad[x] >= 10:
                self.bad[x] |= BAD_ORDER10; count += 1; l_bad[x] = 0
        self.out.append("MB  %d with >=10 bad overlaps\n" % count)
        prune()
        count = 0
        for x in range(1, n + 1):
            if l_bad[x] >= 2:
                self.bad[x] |= BAD_ORDER1; count += 1; l_bad[x] = 0
        self.out.append("MB  %d with multiple bad overlaps\n" % count)
        prune()
        count = 0
        for x in range(1, n + 1):
            if l_bad[x] > 0:
                self.bad[x] |= BAD_ORDER1; count += 1; l_bad[x] = 0
        self.out.append("MB  %d with single bad overlaps\n" % count)

    def mark_contained(self):
        n_con = n_not = tot = 0
        for x in range(1, self.n + 1):
            if self.bad[x]:
                continue
            max_hit = 0
            for iy, n_hit, _, _, flags in self.find_overlaps(x, 0):
                if iy == x or not (flags & F_CONTAINED) or n_hit <= max_hit:
                    continue
                self.contained[x], max_hit = iy, n_hit
            if self.contained[x]:
                n_con += 1
            else:
                n_not += 1; tot += int(self.a["len"][x - 1])
        self.out.append("MC  found %d contained reads, leaving %d not contained, av length %.1f\n" % (n_con, n_not, tot / n_not if n_not else 0.))

    def run(self, cmds):
        """the overlap commands of a modasm command line, in order (-w and its argument are the caller's)"""
        i = 0
        while i < len(cmds):
            c = cmds[i]
            if c == "-o1":
                self.find_overlaps(int(cmds[i + 1]), 2); i += 2
            elif c == "-o2":
                self.overlap_stats(int(cmds[i + 1])); i += 2
            elif c == "-b":
                self.mark_bad_reads(); i += 1
            elif c == "-c":
                self.mark_contained(); i += 1
            else:
                raise ValueError(c)
        return "".join(self.out)


# ---- helpers shared with the GPU tests ----

def golden_stem(golden_dir, tag):
    return os.path.join(golden_dir, "ovl_%s" % tag)


def sequences(tag):
    """{name: (the stem's suffix it reads from, the overlap commands, whether it ends with -w <stem>_BC)} and the generator's read names"""
    j = json.loads(util.golden_text("ovl_%s.sequences.json" % tag))
    out = {}
    for name, cmd in j["sequences"].items():
        writes = "-w" in cmd
        out[name] = ("_BC" if name in j["reads_from"] else "", cmd[:cmd.index("-w")] if writes else cmd, writes)
    return out, j["names"]


def golden_out(tag, name):
    return util.golden_text("ovl_%s.%s.stdout.txt" % (tag, name))


def file_flags(raw):
    """(bad[0..nReads], contained[0..nReads]) of the bytes of a .readset (modasm.c:30-57: records of 72 bytes, bad at 24, contained at 32)"""
    n_max = int.from_bytes(raw[40:44], "little")
    return ([raw[48 + 72 * i + 24] for i in range(n_max)], [int.from_bytes(raw[48 + 72 * i + 32:48 + 72 * i + 36], "little", signed=True) for i in range(n_max)])


def ms_info(ms):
    return mg.modset_arrays(ms)[2]


def lib_flags(rs):
    n = rs.contents.nReads
    return [0] + [int(rs.contents.bad[i]) for i in range(1, n + 1)], [0] + [int(rs.contents.contained[i]) for i in range(1, n + 1)]


def lib_run(rs, cmds, path):
    """the commands through the library, every line into the file `path`; returns the text"""
    with mg.CFile(path, "w") as f:
        i = 0
        while i < len(cmds):
            c = cmds[i]
            if c == "-o1":
                mg.readset_find_overlaps(rs, [int(cmds[i + 1])], 2, f); i += 2
            elif c == "-o2":
                mg.readset_overlap_stats(rs, int(cmds[i + 1]), f); i += 2
            elif c == "-b":
                mg.readset_mark_bad_reads(rs, f); i += 1
            elif c == "-c":
                mg.readset_mark_contained(rs, f); i += 1
            elif c == "-S":
                mg.lib().mgReadsetStats(rs, f); i += 1
            else:
                raise ValueError(c)
    return open(path).read()


class host_loops:
    """MODGPU_READSET_HOST=1 around a block: the records by the library's host loops"""
    def __enter__(self):
        os.environ["MODGPU_READSET_HOST"] = "1"; mg.lib().mgReloadKnobs()

    def __exit__(self, *a):
        del os.environ["MODGPU_READSET_HOST"]; mg.lib().mgReloadKnobs()


def check_sequences_through_library(tag, golden_dir, tmp_path, want_path):
    """every recorded sequence, one fresh load each: the reference's lines; after "bc" the files it wrote"""
    L = mg.lib()
    seqs, _ = sequences(tag)
    stem = golden_stem(golden_dir, tag)
    for name, (suffix, cmds, writes) in seqs.items():
        rs = L.mgReadsetLoad((stem + suffix).encode())
        got = lib_run(rs, cmds, str(tmp_path / "o.txt"))
        assert got == golden_out(tag, name), name
        assert L.mgReadsetOverlapsPath() == want_path, name
        if writes:
            out = str(tmp_path / "bc")
            L.mgReadsetWrite(rs, out.encode())
            assert gzip.open(out + ".mod").read() == gzip.open(stem + "_BC.mod").read()
            assert trs.readset_mask(gzip.open(out + ".readset").read()) == trs.readset_mask(gzip.open(stem + "_BC.readset").read())
        L.mgReadsetDestroy(rs)


# ---- the tests ----

@pytest.mark.parametrize("tag", list(TAGS))
def test_restatement_vs_reference_program(tag, golden_dir):
    """every recorded command sequence: the reference's lines, and after -b -c the flags of the file it wrote"""
    L = mg.lib()
    seqs, _ = sequences(tag)
    stem = golden_stem(golden_dir, tag)
    bad_bc, con_bc = file_flags(gzip.open(stem + "_BC.readset").read())
    assert any(bad_bc) and any(con_bc)
    rs = L.mgReadsetLoad(stem.encode())
    a, info = trs.lib_arrays(rs), ms_info(rs.contents.ms)
    assert len(seqs) == len(a["nHit"]) + 6
    for name, (suffix, cmds, writes) in seqs.items():
        if "-S" in cmds:
            continue                                                  # -S is the library's: below
        r = Restatement(a, info, *((bad_bc, con_bc) if suffix else ()))
        assert r.run(cmds) == golden_out(tag, name), name
        if writes:
            assert (r.bad, r.contained) == (bad_bc, con_bc)
    L.mgReadsetDestroy(rs)


@pytest.mark.parametrize("tag", list(TAGS))
def test_host_loops_vs_reference_program(tag, golden_dir, tmp_path):
    with host_loops():
        check_sequences_through_library(tag, golden_dir, tmp_path, 1)


@pytest.mark.parametrize("tag", list(TAGS))
def test_flags_survive_load_and_write(tag, golden_dir, tmp_path):
    """load-then-write of ovl_<tag>_BC returns its bytes, bad and contained included; create and ingest leave zeros"""
    L = mg.lib()
    stem = golden_stem(golden_dir, tag) + "_BC"
    rs = L.mgReadsetLoad(stem.encode())
    want = file_flags(gzip.open(stem + ".readset").read())
    assert lib_flags(rs) == want and any(want[0]) and any(want[1])
    out = str(tmp_path / "again")
    L.mgReadsetWrite(rs, out.encode())
    assert gzip.open(out + ".mod").read() == gzip.open(stem + ".mod").read()
    assert trs.readset_mask(gzip.open(out + ".readset").read()) == trs.readset_mask(gzip.open(stem + ".readset").read())
    assert file_flags(gzip.open(out + ".readset").read()) == want
    L.mgReadsetDestroy(rs)
    rs0 = L.mgReadsetLoad(golden_stem(golden_dir, tag).encode())
    assert not any(lib_flags(rs0)[0]) and not any(lib_flags(rs0)[1])
    L.mgReadsetDestroy(rs0)


@pytest.mark.parametrize("tag", list(TAGS))
def test_overlap_lists_vs_restatement(tag, golden_dir, tmp_path):
    """MgOverlaps for every read in one call, then after -b: entries, their order inside ties, the skipped ones"""
    L = mg.lib()
    rs = L.mgReadsetLoad(golden_stem(golden_dir, tag).encode())
    a, info = trs.lib_arrays(rs), ms_info(rs.contents.ms)
    n = len(a["nHit"])
    r = Restatement(a, info)
    with host_loops():
        for round_ in range(2):
            want = [r.find_overlaps(x, 0) for x in range(1, n + 1)]
            got = mg.readset_find_overlaps(rs, list(range(1, n + 1)), 0, None, want_lists=True)
            assert got == want
            assert lib_flags(rs)[0] == r.bad
            if round_ == 0:
                assert any(len({e[1] for e in l}) < len(l) for l in want)                 # ties in nHit
                assert any(e[4] & F_SKIPPED for l in want for e in l)
                r.mark_bad_reads(); lib_run(rs, ["-b"], str(tmp_path / "b.txt"))
        # a read given twice, and a read after itself: the replay is in the order given
        want = [r.find_overlaps(x, 0) for x in (5, 5, 1)]
        assert mg.readset_find_overlaps(rs, [5, 5, 1], 0, None, want_lists=True) == want
    L.mgReadsetDestroy(rs)


# ---- read sets built by design (tests/overlap_designs.py): the oracle writes them, the library loads them, the host loops run ----

@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_designed_sets_through_the_host_loops(name, tmp_path):
    """set A (strides of 64 hits), B (copy classes), C (table sizes), D (many pairs, ties), E (positions past 2^16), each with its properties
    asserted from the restatement (overlap_designs.check_*), written by the oracle, loaded by mgReadsetLoad and run by ovlBatchHost / ovlPairHost:
    lists, -o2 / -b / -c lines and flags against the restatement; B under exact candidate budgets, D's subsets and a query list of more than 1024"""
    from tests import overlap_designs as od
    stem = str(tmp_path / ("set" + name))
    a, info = od.oracle_set(name, stem)
    rs = mg.lib().mgReadsetLoad(stem.encode())
    trs.same(trs.lib_arrays(rs), a)
    assert np.array_equal(ms_info(rs.contents.ms), info)
    r0 = od.checked(name, a, info)
    with host_loops():
        od.run_set(name, rs, r0, tmp_path, 1)
    mg.lib().mgReadsetDestroy(rs)


def test_error_cases(golden_dir, tmp_path):
    """what the reference cannot do comes back as -1 with a message: a read number outside 1 .. nReads, an active copy-1 mod whose depth
    saturated (no inverse list: modasm.c:266,338), a read of more than 65534 hits (U16 hmap / nHit, modasm.c:293,320)"""
    L = mg.lib()
    tag = list(TAGS)[0]
    with host_loops():
        rs = L.mgReadsetLoad(golden_stem(golden_dir, tag).encode())
        n = rs.contents.nReads
        for bad_no in (0, n + 1, 0xffffffff):
            with pytest.raises(mg.ModgpuError, match="read"):
                mg.readset_find_overlaps(rs, [1, bad_no], 1, None)
        with pytest.raises(mg.ModgpuError):
            mg.readset_overlap_stats(rs, 0, None)
        assert not any(lib_flags(rs)[0])                                             # nothing was replayed
        # saturated depth on a copy-1 mod that read 1 holds
        ms = rs.contents.ms
        m = int(rs.contents.hit[int(rs.contents.hitStart[1]) + 3]) & TOPMASK
        assert (int(ms.contents.info[m]) & 3) == 1
        old = ms.contents.depth[m]
        ms.contents.depth[m] = 0xffff
        with pytest.raises(mg.ModgpuError, match="depth"):
            mg.readset_find_overlaps(rs, [1], 1, None)
        with pytest.raises(mg.ModgpuError, match="depth"):
            lib_run(rs, ["-b"], str(tmp_path / "b.txt"))
        ms.contents.depth[m] = old
        assert lib_run(rs, ["-o1", "1"], str(tmp_path / "o.txt")) == golden_out(tag, "o1_1")
        L.mgReadsetDestroy(rs)
        # a read of 65535 hits: the struct says so, the lists are never walked
        rs = L.mgReadsetLoad(golden_stem(golden_dir, tag).encode())
        old = rs.contents.nHit[2]
        rs.contents.nHit[2] = 65535
        with pytest.raises(mg.ModgpuError, match="65534"):
            mg.readset_find_overlaps(rs, [1], 1, None)
        rs.contents.nHit[2] = old
        L.mgReadsetDestroy(rs)


def test_names_in_header_library_and_binding():
    header = open(os.path.join(util.ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n in NAMES:
        assert re.search(r"^int  %s \(" % n, header, re.M), n
    for n in VOID_NAMES:
        assert re.search(r"^void %s \(" % n, header, re.M), n
    for n in NAMES + VOID_NAMES:
        assert n in mg.EXPORTS and hasattr(L, n), n
    assert re.search(r"U8 \*bad ; int \*contained ;", header) and "MgOverlaps" in header
    assert [f[0] for f in mg.MgReadset._fields_][-2:] == ["bad", "contained"]
    for f in ("readset_find_overlaps", "readset_overlap_stats", "readset_mark_bad_reads", "readset_mark_contained", "readset_overlaps_diag"):
        assert callable(getattr(mg, f)), f
    assert "mg_overlap.o" in open(os.path.join(util.ROOT, "modimizer_amd", "csrc", "Makefile")).read()
