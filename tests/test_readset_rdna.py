"""modasm -R / -T / -rb (refFlag, modasm.c:752-860; testMods, 595-748; resetBits, 864-908): a plain Python restatement of the three passes against the
reference program's own output for every recorded command sequence (tests/golden/rdna_*: make_golden_rdna.py) -- stdout, YY-TEST*, ZZ-TEST*, the
written .mod and .readset -- which the designed and randomized GPU tests (test_gpu_readset_rdna.py) then lean on; the library's host loops
(MODGPU_READSET_HOST=1, the reference sequence's hits fed through mgReadsetRefFlagHits) against the same; the refusals; the names in header, library
and binding.

The reference file with an N (rdna_<tag>_refN.fa): the reference maps N to 0 only after a -f in the same process (modasm.c:159); in the recorded
`-r stem -R` case it hashes a base 4.  The library reads N as base 0.  The fixture's N lies where both give the same hits (the maker asserts it), and
the sequence "RN" pins that case."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import modimizer_amd as mg
from modimizer_amd import fasta
from tests import util
from tests import test_readset as trs
from tests.test_readset_overlap import host_loops, ms_info

TAGS = {"k19d8": (19, 8)}
TOPMASK, TOPBIT = 0x7fffffff, 0x80000000
MS_REPEAT, MS_RDNA = 8, 0x20
REF, CORE, VAR, MULTI = 1, 2, 4, 8
NAMES = ["mgReadsetRefFlagFile", "mgReadsetRefFlagHits", "mgReadsetResetBits", "mgReadsetTestMods", "mgReadsetTestModsRun", "mgReadsetRdnaPath"]
HOOKS = ["mgReadsetRdnaDiag", "mgReadsetRdnaGrid"]


class Refused(Exception):
    """what the reference cannot do: the library returns -1 there"""


def check_mod(info):
    return (info & 3) != 0 and (info & (MS_REPEAT | MS_RDNA)) == MS_RDNA


def depth_class(d):
    return MULTI if d > 4750 else CORE if d > 2750 else VAR


# ---- the restatement: a = test_readset.lib_arrays (reads from 0 there), info / depth = the set's arrays, w = the hasher's w ----

class Rdna:
    def __init__(self, a, info, depth, w, read_flags=None):
        self.a, self.w = a, w
        self.info = [int(v) for v in info]
        self.depth = [int(v) for v in depth]
        self.m = len(self.info)
        self.n = len(a["nHit"])
        self.hs = [int(v) for v in a["hitStart"]]
        self.hit = np.asarray(a["hit"], dtype=np.int64)
        self.mod = self.hit & TOPMASK
        self.fwd = (self.hit & TOPBIT) != 0
        self.pos = np.zeros(len(self.hit), np.int64)
        dx = np.asarray(a["dx"], dtype=np.int64)
        for i in range(self.n):
            self.pos[self.hs[i]:self.hs[i + 1]] = np.cumsum(dx[self.hs[i]:self.hs[i + 1]])
        self.len = [int(v) for v in a["len"]]
        self.inv_start, self.inv = [int(v) for v in a["invStart"]], [int(v) for v in a["invSpace"]]
        self.mi = None                                                # per mod [flags, rDNApos, nGood, nMod2, nBadLD, nSplit, nSplitLD]
        self.read_flags = [0] * (self.n + 1) if read_flags is None else list(read_flags)
        self.run_no = 0
        self.out, self.yy, self.zz = [], {}, {}
        self.diag = None
        # what the last -T saw, for the designed sets (tests/rdna_designs.py): the tested mods; per tested mod the extents of its start and end array,
        # the cells of either that a visit counted in, its partners, and per visit (read, hit number of i's first occurrence in it, forward)
        self.tested, self.ext, self.start_cells, self.end_cells, self.cell_mods, self.first = None, {}, {}, {}, {}, {}

    def n_copy(self):
        info = np.array(self.info, np.int64) & 3
        return [[int((info[self.mod[self.hs[i]:self.hs[i + 1]]] == c).sum()) for c in range(4)] for i in range(self.n)]

    # -- -R --
    def ref_flag_hits(self, index, pos):
        if self.mi is None:
            self.mi = [[0, 0, 0, 0, 0, 0, 0] for _ in range(self.m)]
        mi = self.mi
        for ix, p in zip(index, pos):
            ix = int(ix)
            self.info[ix] |= MS_RDNA
            mi[ix][0] |= REF | depth_class(self.depth[ix]); mi[ix][1] = int(p)
        qual = np.array([(q[0] & (REF | CORE)) == (REF | CORE) for q in mi])
        r_count = {}
        n_rdna_reads = 0
        for i in range(1, self.n + 1):
            mods = self.mod[self.hs[i - 1]:self.hs[i]]
            at = np.flatnonzero(qual[mods]) if len(mods) else np.zeros(0, np.int64)
            n200 = int(at[199]) if len(at) >= 200 else 0
            m200 = 0
            if n200:
                back = at[at >= 1]                                     # the loop from the back never looks at hit 0
                m200 = int(back[len(back) - 200]) if len(back) >= 200 else 0
            if m200 <= n200:
                continue
            last = 0
            for j in range(n200, m200):
                h = int(mods[j]); q = mi[h]
                if q[0]:
                    p = q[1]
                    if q[0] & REF:
                        last = p
                    elif p > 0 and last - 50 < p < last + 50:
                        c = r_count.get(h, 0)
                        q[1] = int((c * p + last) / (c + 1)) if (c * p + last) >= 0 else -int(-(c * p + last) / (c + 1))
                        r_count[h] = c + 1
                    else:
                        q[1] = -1
                else:
                    self.info[h] |= MS_RDNA; q[0] |= depth_class(self.depth[h]); q[1] = last; r_count[h] = 1
            self.read_flags[i] |= 1; n_rdna_reads += 1
        c = dict.fromkeys("nRDNA nRef nGoodPos nRefC nRefV0 nRefV1 nRefM nOthC nOthV0 nOthV1 nOthM".split(), 0)
        for i, q in enumerate(mi):
            if not q[0]:
                continue
            c["nRDNA"] += 1
            kind = "C" if q[0] & CORE else "M" if q[0] & MULTI else "V0" if (self.info[i] & 3) == 0 else "V1"
            if q[0] & REF:
                c["nRef"] += 1; c["nRef" + kind] += 1
            else:
                c["nOth" + kind] += 1
                c["nGoodPos"] += q[1] > 0
        self.out.append("total nRDNAreads %d other reads %d\n" % (n_rdna_reads, self.n - n_rdna_reads))
        self.out.append("total nRDNAmods %d nRDNAref %d other mods %d\n" % (c["nRDNA"], c["nRef"], self.m - c["nRDNA"]))
        self.out.append("  nRefC %d nRefM %d nRefVcopy>0 %d nRefVcopy0 %d\n" % (c["nRefC"], c["nRefM"], c["nRefV1"], c["nRefV0"]))
        self.out.append("  nOthC %d nOthM %d nOthVcopy>0 %d nOthVcopy0 %d nGoodPos %d\n" % (c["nOthC"], c["nOthM"], c["nOthV1"], c["nOthV0"], c["nGoodPos"]))

    # -- -rb --
    def reset_bits(self, op):
        if self.mi is None:
            raise Refused("-rb before -R")
        if op not in (1, 2, 3):
            return
        if op == 3 and self.n < 1:
            raise Refused("-rb 3 on an empty set")
        n = 0
        for i, q in enumerate(self.mi):
            if (q[0] & CORE) and not (op == 2 and self.info[i] & MS_REPEAT):
                self.info[i] = (self.info[i] & 0xfc) | 1; n += 1
            else:
                self.info[i] &= 0xfc
        head = {1: "resetting rDNA core kmers to copy1, rest to copy0:", 2: "resetting non-repetitive rDNA core kmers to copy1, rest to copy0:",
                3: "resetting rDNA core kmers not repeated in read 1 to copy1: "}[op]
        if op == 3:
            seen = set()
            for h in self.mod[self.hs[0]:self.hs[1]]:
                h = int(h)
                if (self.info[h] & 3) != 1:
                    continue
                if h in seen:
                    self.info[h] &= 0xfc; n -= 1
                else:
                    seen.add(h)
        self.out.append("%s %d kept\n" % (head, n))

    # -- -T --
    def test_mods(self, lo, hi):
        if self.mi is None:
            raise Refused("need to run -R first")
        run = self.run_no + 1
        chk = np.array([check_mod(v) for v in self.info])
        tested = [i for i in range(self.m) if lo <= self.depth[i] < hi and chk[i]]
        if not tested:
            raise Refused("no mod tested: arrayDestroy (0)")
        for i in tested:
            if self.depth[i] in (0, 0xffff):
                raise Refused("tested mod without a list")
        res, bad_ld, split_ld = {}, [0] * self.m, [0] * self.m
        zz, visits, occ, big = [], 0, 0, [0, 0]
        cnt, mn, mx = np.zeros(self.m, np.int64), np.zeros(self.m, np.int64), np.zeros(self.m, np.int64)
        self.tested, self.ext, self.start_cells, self.end_cells, self.cell_mods, self.first = tested, {}, {}, {}, {}, {}
        for i in tested:
            start, end = {}, {}
            self.first[i] = []
            cnt[:] = 0; mn[:] = 1 << 40; mx[:] = -(1 << 40)
            # a read that holds i more than once is visited once per occurrence, every time from the FIRST occurrence: the same contribution each time
            rd, times = np.unique(np.array(self.inv[self.inv_start[i]:self.inv_start[i] + self.depth[i]], np.int64), return_counts=True)
            for r, t in zip(rd.tolist(), times.tolist()):
                visits += t
                h0, h1 = self.hs[r - 1], self.hs[r]
                mods = self.mod[h0:h1]
                f = int(np.argmax(mods == i))
                assert mods[f] == i
                x = int(self.pos[h0 + f]); o = self.len[r - 1] - x - self.w
                if o < 0:
                    raise Refused("len - x - w < 0")
                fw = bool(self.fwd[h0 + f])
                self.first[i] += [(r, f, fw)] * t
                s, e = (x, o) if fw else (o, x)
                start[s] = start.get(s, 0) + t; end[e] = end.get(e, 0) + t
                d = self.pos[h0:h1] - x if fw else x - self.pos[h0:h1]
                keep = chk[mods]; keep[f] = False
                np.add.at(cnt, mods[keep], t); np.minimum.at(mn, mods[keep], d[keep]); np.maximum.at(mx, mods[keep], d[keep])
            cells = {int(m_): (int(cnt[m_]), int(mn[m_]), int(mx[m_])) for m_ in np.flatnonzero(cnt)}
            self.cell_mods[i], self.start_cells[i], self.end_cells[i] = sorted(cells), sorted(start), sorted(end)
            def suffix(t):
                ext = max(t) + 1
                a = [0] * ext
                for k_, v in t.items():
                    a[k_] = v
                for k_ in range(ext - 2, -1, -1):
                    a[k_] += a[k_ + 1]
                return a
            start, end = suffix(start), suffix(end)
            self.ext[i] = (len(start), len(end))
            for y, arr in enumerate((start, end)):                     # arrayReCreate clears 20000 cells of an array that is there (array.c:103): stale cells from the second such mod on
                big[y] += len(arr) > 20000
                if big[y] > 1:
                    raise Refused("stale cells beyond 20000")
            n_good = n_mod2 = n_split = 0
            for m_ in sorted(cells):
                n, dmin, dmax = cells[m_]
                occ += n
                if dmin > 0:
                    xmin, xmax, arr, sign = dmin, dmax, end, "+"
                else:
                    xmax, xmin, arr, sign = -dmin, -dmax, start, "-"
                    if xmin < 0:
                        n_split += 1; split_ld[m_] += 1; xmin = xmax
                if xmin >= len(arr) or xmax >= len(arr):
                    raise Refused("a distance beyond the array")
                v = arr[xmin]
                if n < self.depth[m_] and n * 2 < v:
                    n_mod2 += 1
                    if run > 3:
                        bad_ld[m_] += 1
                elif sign == "-" and n == 1 and v >= 10:
                    bad_ld[m_] += 1
                if n == self.depth[m_] or n >= 0.8 * v:
                    n_good += 1
                if sign == "+" and n == 1 and v >= 10:
                    bad_ld[i] += 1
                zz.append("i %d depth %d m %d depth %d %s count %d min %d at %d max %d at %d\n" % (i, self.depth[i], m_, self.depth[m_], sign, n, v, xmin, arr[xmax], xmax))
            res[i] = (n_good, n_mod2, n_split)
        # nothing was modified so far: commit
        for i, q in enumerate(self.mi):
            q[2:] = [0, 0, bad_ld[i], 0, split_ld[i]]
        for i, (g, m2, sp) in res.items():
            self.mi[i][2], self.mi[i][3], self.mi[i][5] = g, m2, sp
        yy, z1, z2, z3 = [], 0, 0, 0
        for i, q in enumerate(self.mi):
            _, _, n_good, n_mod2, n_bad, n_split, n_split_ld = q
            def zero():
                self.info[i] &= 0xfc
            def badld():
                yy.append("BADLD %d depth %d nBadLD %d nSplitLD %d\n" % (i, self.depth[i], n_bad, n_split_ld)); zero()
            if n_good or n_mod2:
                yy.append("TEST %d depth %d nGood %d nMod2 %d nBadLD %d nSplit %d\n" % (i, self.depth[i], n_good, n_mod2, n_bad, n_split))
            if n_good < n_mod2:
                zero(); z1 += 1
            if n_split > 10:
                zero(); z2 += 1
            if run in (2, 6) and (n_bad > 20 or n_split_ld > 10):
                badld(); z3 += 1
            if run in (3, 7):
                if n_mod2 > 25:
                    zero(); z1 += 1
                if n_split:
                    zero(); z2 += 1
                if n_bad > 10:
                    badld(); z3 += 1
            if run in (4, 8):
                if n_bad > 6 and n_split:
                    zero(); z2 += 1
                badld(); z3 += 1                                       # the braces of modasm.c:735-738 belong to no `if`: every mod
        self.run_no = run
        self.yy[str(run)], self.zz[str(run)] = "".join(yy), "".join(zz)
        self.out.append("RUN %d tested %d mods and zeroed %d bad>good %d split %d LD\n" % (run, len(tested), z1, z2, z3))
        self.diag = (len(tested), visits, occ)


# ---- helpers shared with the GPU tests ----

def golden_stem(golden_dir, tag):
    return os.path.join(golden_dir, "rdna_%s" % tag)


def sequences(tag):
    return json.loads(util.golden_text("rdna_%s.sequences.json" % tag))


def golden_out(golden_dir, tag, name):
    return json.loads(gzip.open(golden_stem(golden_dir, tag) + ".%s.json.gz" % name).read())


_ref_hits = {}


def ref_hits(rs, path, k, w):
    """(index, pos) of the sequences of the FASTA file `path` in the set of rs, in file order, misses left out: the oracle's scan, N as base 0"""
    key = (path, k, w)
    if key not in _ref_hits:
        from oracle import pyoracle as po
        values = mg.modset_arrays(rs.contents.ms)[0]
        where = {int(v): i for i, v in enumerate(values) if i}
        h = po.Hasher(k, w, 17)
        ix, ps = [], []
        for s in fasta.read_fasta_list(path):
            km, pos, _ = h.scan(s)
            for v, p in zip(km.tolist(), pos.tolist()):
                if v in where:
                    ix.append(where[v]); ps.append(p)
        _ref_hits[key] = (np.array(ix, np.uint32), np.array(ps, np.int32))
    return _ref_hits[key]


def strip_stats(text):
    """the lines of the commands these tests restate: -S's and -C's belong to other tests"""
    return "".join(l + "\n" for l in text.splitlines() if l.startswith(("total n", "  nRef", "  nOth", "resetting", "RUN ")))


def restatement_run(r, cmds, hits_of):
    """the -R / -T / -rb / -C commands of a modasm command line on the restatement `r`; hits_of (file) -> (index, pos); -C through `clean` if given.
    Returns the refusal's text if one of them was refused, else None"""
    i = 0
    try:
        while i < len(cmds):
            c = cmds[i]
            if c == "-R":
                r.ref_flag_hits(*hits_of(cmds[i + 1])); i += 2
            elif c == "-T":
                r.test_mods(int(cmds[i + 1]), int(cmds[i + 2])); i += 3
            elif c == "-rb":
                r.reset_bits(int(cmds[i + 1])); i += 2
            elif c == "-C":
                clean_mods(r); i += 1
            elif c == "-S":
                i += 1
            elif c == "-w":
                i += 2
            else:
                raise ValueError(c)
    except Refused as e:
        return str(e)
    return None


def clean_mods(r):
    """cleanMods' repeat flag (modasm.c:529-532) on the restatement: the other two flags of -C do not enter checkMod.  The last read is not looked at"""
    for i in range(1, r.n):
        mods = r.mod[r.hs[i - 1]:r.hs[i]]
        u, c = np.unique(mods, return_counts=True)
        for h in u[c > 1].tolist():
            r.info[h] |= MS_REPEAT


def lib_run(rs, cmds, tmp, hits_of=None, want_z=True):
    """the commands through the library; -R through mgReadsetRefFlagHits when hits_of is given (no device needed), else through the file.  Returns
    (stdout text, {run: YY}, {run: ZZ}, the refusal's message or None)"""
    L = mg.lib()
    yy, zz, err = {}, {}, None
    out_path = os.path.join(tmp, "out.txt")
    with mg.CFile(out_path, "w") as f:
        i = 0
        try:
            while i < len(cmds):
                c = cmds[i]
                if c == "-R":
                    if hits_of is None:
                        mg.readset_ref_flag(rs, cmds[i + 1], f)
                    else:
                        mg.readset_ref_flag_hits(rs, *hits_of(cmds[i + 1]), f)
                    i += 2
                elif c == "-T":
                    run = L.mgReadsetTestModsRun(rs) + 1
                    yp, zp = os.path.join(tmp, "YY-TEST%d" % run), os.path.join(tmp, "ZZ-TEST%d" % run)
                    with mg.CFile(yp, "w") as y, mg.CFile(zp, "w") as z:
                        mg.readset_test_mods(rs, int(cmds[i + 1]), int(cmds[i + 2]), f, y, z if want_z else None)
                    yy[str(run)], zz[str(run)] = open(yp).read(), open(zp).read()
                    i += 3
                elif c == "-rb":
                    mg.readset_reset_bits(rs, int(cmds[i + 1]), f); i += 2
                elif c == "-C":
                    L.mgReadsetCleanMods(rs, f); i += 1
                elif c == "-S":
                    L.mgReadsetStats(rs, f); i += 1
                elif c == "-w":
                    i += 2
                else:
                    raise ValueError(c)
        except mg.ModgpuError as e:
            err = str(e)
    return open(out_path).read(), yy, zz, err


def mod_info_rows(rs):
    v = mg.readset_mod_info(rs)
    return None if v is None else [[int(x) for x in row] for row in v.tolist()]


def check_sequences_through_library(tag, golden_dir, tmp_path, want_path, hits=True):
    """every recorded sequence, one fresh load each: the reference's stdout, YY and ZZ files; after "w" the files it wrote"""
    L = mg.lib()
    k, w = TAGS[tag]
    j = sequences(tag)
    stem = golden_stem(golden_dir, tag)
    for name, cmds in j["sequences"].items():
        g = golden_out(golden_dir, tag, name)
        rs = L.mgReadsetLoad((os.path.join(golden_dir, j["reads_from"][name]) if name in j["reads_from"] else stem).encode())
        hits_of = (lambda f: ref_hits(rs, os.path.join(golden_dir, f), k, w)) if hits else None
        cmds = [os.path.join(golden_dir, c) if c.endswith(".fa") and not hits else c for c in cmds]
        d = tmp_path / name; d.mkdir()
        out, yy, zz, err = lib_run(rs, cmds, str(d), hits_of)
        if g["rc"]:
            assert err is not None, name
            if "need to run -R first" in g["stderr"]:
                assert "need to run -R first" in err
            assert strip_stats(g["stdout"]).startswith(strip_stats(out)), name          # what it printed before it died
            if name in j["reads_from"]:
                assert mg.readset_read_flags(rs).sum() > 0                              # otherFlags came with the file
        else:
            assert err is None, (name, err)
            assert out == g["stdout"], name
            assert yy == g["YY"] and zz == g["ZZ"], name
            assert L.mgReadsetRdnaPath() == want_path, name
        if "-w" in cmds:
            o = str(d / "w")
            L.mgReadsetWrite(rs, o.encode())
            wrote = os.path.join(golden_dir, cmds[cmds.index("-w") + 1])
            assert gzip.open(o + ".mod").read() == gzip.open(wrote + ".mod").read()
            assert trs.readset_mask(gzip.open(o + ".readset").read()) == trs.readset_mask(gzip.open(wrote + ".readset").read())
        L.mgReadsetDestroy(rs)


# ---- read sets made by design: a .mod from the library's host API with depth[] / info[] as given, a .readset written here ----

REC = np.dtype([("len", "<i4"), ("nHit", "<i4"), ("hitPtr", "<u8"), ("dxPtr", "<u8"), ("bad", "u1"), ("otherFlags", "u1"), ("pad1", "<u2"), ("nMiss", "<i4"),
                ("contained", "<i4"), ("nCopy", "<i4", 4), ("pad2", "<u4", 4), ("tail", "<u4")])
assert REC.itemsize == 72


def build_set(stem, k, w, n_mods, reads, info, depth=None):
    """mgReadsetLoad of a set made here: mods 1 .. n_mods; reads = [(length, [(mod, forward, dx), ...]), ...]; info[0 .. n_mods]; depth: the hits per mod
    unless given.  The caller destroys rs and rs.contents.ms"""
    L = mg.lib()
    ms = mg.modsetCreate(mg.seqhashCreate(k, w, 17), 20)
    for i in range(1, n_mods + 1):
        assert L.modsetIndexFind(ms, 5 * i + 1, 1) == i
    count = np.zeros(n_mods + 1, np.int64)
    for _, hits in reads:
        for m, _, _ in hits:
            count[m] += 1
    dep = np.minimum(count, 0xffff) if depth is None else np.asarray(depth)
    for i in range(n_mods + 1):
        ms.contents.depth[i] = int(dep[i]); ms.contents.info[i] = int(info[i])
    with mg.CFile(stem + ".mod", "w") as f:
        L.modsetWrite(ms, f)
    L.modsetDestroy(ms)
    recs = np.zeros(len(reads) + 1, REC)
    tot = sum(len(h) for _, h in reads)
    body = []
    for i, (length, hits) in enumerate(reads):
        recs[i + 1]["len"], recs[i + 1]["nHit"] = length, len(hits)
        if hits:
            body.append(np.array([m | (TOPBIT if fw else 0) for m, fw, _ in hits], "<u4").tobytes())
            body.append(np.array([d for _, _, d in hits], "<u2").tobytes())
    head = np.array([8918274, 0], "<i4").tobytes() + bytes(8) + np.array([len(recs), 72, len(recs), 0], "<i4").tobytes()
    open(stem + ".readset", "wb").write(b"RSMSHv2\0" + np.array([tot], "<u8").tobytes() + head + recs.tobytes() + b"".join(body))
    return L.mgReadsetLoad(stem.encode())


def destroy(rs):
    """a set from build_set or mgReadsetLoad with the modset that came with it (a pointer of its own: rs.contents.ms lives in the struct that goes)"""
    import ctypes
    ms = ctypes.cast(rs.contents.ms, ctypes.POINTER(mg.Modset))
    mg.lib().mgReadsetDestroy(rs); mg.lib().modsetDestroy(ms)


def restatement_of(rs):
    ms = rs.contents.ms
    _, depth, info = mg.modset_arrays(ms)
    r = Rdna(trs.lib_arrays(rs), info, depth, ms.contents.hasher.contents.w, mg.readset_read_flags(rs))
    r.mi, r.run_no = mod_info_rows(rs), mg.lib().mgReadsetTestModsRun(rs)          # what -R and -T have left beside the set so far
    return r


def same_state(rs, r):
    """the library's set against the restatement: info[], ModInfo, the reads' flags, nCopy[], the -T count"""
    assert [int(v) for v in ms_info(rs.contents.ms)] == r.info
    assert mod_info_rows(rs) == r.mi
    assert mg.readset_read_flags(rs).tolist() == r.read_flags
    assert trs.lib_arrays(rs)["nCopy"].tolist() == r.n_copy()
    assert mg.lib().mgReadsetTestModsRun(rs) == r.run_no


def run_both(rs, cmds, tmp, hits):
    """cmds through the library and through the restatement, -R from hits = (index, pos): lines, files, state and refusals agree.  Returns the restatement"""
    r = restatement_of(rs)
    hits_of = lambda _f: hits
    want_err = restatement_run(r, cmds, hits_of)
    out, yy, zz, err = lib_run(rs, cmds, tmp, hits_of)
    assert (err is None) == (want_err is None), (err, want_err)
    assert out == "".join(r.out) and yy == r.yy and zz == r.zz
    same_state(rs, r)
    return r


# ---- the tests ----

@pytest.mark.parametrize("tag", list(TAGS))
def test_restatement_vs_reference_program(tag, golden_dir):
    """every recorded command sequence: the reference's lines and files; after -w the flags, info[] and nCopy[] of the files it wrote"""
    L = mg.lib()
    k, w = TAGS[tag]
    j = sequences(tag)
    stem = golden_stem(golden_dir, tag)
    rs = L.mgReadsetLoad(stem.encode())
    rw = L.mgReadsetLoad((stem + "_W").encode())
    hits_of = lambda f: ref_hits(rs, os.path.join(golden_dir, f), k, w)
    assert len(hits_of(j["refs"]["_ref"])[0]) > 20 and np.array_equal(hits_of(j["refs"]["_ref"])[0], hits_of(j["refs"]["_refN"])[0])
    runs_seen = set()
    for name, cmds in j["sequences"].items():
        g = golden_out(golden_dir, tag, name)
        r = restatement_of(rw if name in j["reads_from"] else rs)
        refusal = restatement_run(r, cmds, hits_of)
        assert (refusal is not None) == (g["rc"] != 0), (name, refusal)
        if refusal:
            assert strip_stats(g["stdout"]).startswith("".join(r.out)), name
            continue
        assert "".join(r.out) == strip_stats(g["stdout"]), name
        assert r.yy == g["YY"] and r.zz == g["ZZ"], name
        runs_seen |= set(r.yy)
        if name == "w":
            assert r.read_flags == mg.readset_read_flags(rw).tolist() and sum(r.read_flags) > 0
            assert [v & ~0x14 for v in r.info] == [int(v) & ~0x14 for v in ms_info(rw.contents.ms)]      # (-C's internal and minor flags are not restated here)
            assert r.n_copy() == trs.lib_arrays(rw)["nCopy"].tolist()
    assert runs_seen == {str(i) for i in range(1, 9)}
    L.mgReadsetDestroy(rs); L.mgReadsetDestroy(rw)


@pytest.mark.parametrize("tag", list(TAGS))
def test_host_loops_vs_reference_program(tag, golden_dir, tmp_path):
    with host_loops():
        check_sequences_through_library(tag, golden_dir, tmp_path, 1)


@pytest.mark.parametrize("tag", list(TAGS))
def test_other_flags_survive_load_and_write(tag, golden_dir, tmp_path):
    """load-then-write of rdna_<tag>_W returns its bytes, byte 25 of every record included; ModInfo and the -T count do not come with a file"""
    L = mg.lib()
    stem = golden_stem(golden_dir, tag) + "_W"
    raw = gzip.open(stem + ".readset").read()
    want = [raw[48 + 72 * i + 25] for i in range(int.from_bytes(raw[40:44], "little"))]
    rs = L.mgReadsetLoad(stem.encode())
    assert mg.readset_read_flags(rs).tolist() == want and sum(want) > 0
    assert mg.readset_mod_info(rs) is None and L.mgReadsetTestModsRun(rs) == 0
    out = str(tmp_path / "again")
    L.mgReadsetWrite(rs, out.encode())
    assert trs.readset_mask(gzip.open(out + ".readset").read()) == trs.readset_mask(raw)
    L.mgReadsetDestroy(rs)
    rs0 = L.mgReadsetLoad(golden_stem(golden_dir, tag).encode())
    assert not mg.readset_read_flags(rs0).any()
    L.mgReadsetDestroy(rs0)


def small_design(stem, w=8, k=19, info_of=None):
    """three mods of depth 12 in 12 reads, i = 2 between 1 and 3, every read forward"""
    reads = [(400, [(1, True, 50), (2, True, 60), (3, True, 70)]) for _ in range(12)]
    info = [0] + [MS_RDNA | 1] * 3
    if info_of:
        info = info_of(info)
    return build_set(stem, k, w, 3, reads, info)


def test_refusals(tmp_path):
    """-1, with the set as it was: -T and -rb before -R; -rb 3 on an empty set; a tested mod of depth 0 or of saturated depth; a -T that tests no mod (the
    reference dies in arrayDestroy (0) at its end); with w > k a visit with len - x - w < 0, and a distance beyond the count array"""
    L = mg.lib()
    with host_loops():
        rs = small_design(str(tmp_path / "a"))
        hits = (np.array([1], np.uint32), np.array([7], np.int32))
        for call in (lambda: mg.readset_test_mods(rs, 1, 100, None), lambda: mg.readset_reset_bits(rs, 1, None)):
            with pytest.raises(mg.ModgpuError, match="need to run -R first"):
                call()
        with pytest.raises(mg.ModgpuError, match="names mod"):
            mg.readset_ref_flag_hits(rs, [4], [0], None)
        assert mg.readset_mod_info(rs) is None
        mg.readset_ref_flag_hits(rs, *hits, None)
        before = (mod_info_rows(rs), ms_info(rs.contents.ms).tolist())
        ms = rs.contents.ms
        with pytest.raises(mg.ModgpuError, match="no mod"):
            mg.readset_test_mods(rs, 500, 600, None)
        for d in (0, 0xffff):
            ms.contents.depth[2] = d
            with pytest.raises(mg.ModgpuError, match="depth"):
                mg.readset_test_mods(rs, 0, 70000, None)
        ms.contents.depth[2] = 12
        assert (mod_info_rows(rs), ms_info(ms).tolist()) == before and L.mgReadsetTestModsRun(rs) == 0
        run_both(rs, ["-T", "1", "100", "-rb", "7", "-rb", "2"], str(tmp_path), hits)
        destroy(rs)
        # -rb 3 on an empty set
        rs = build_set(str(tmp_path / "e"), 19, 8, 3, [], [0, 1, 1, 1])
        mg.readset_ref_flag_hits(rs, *hits, None)
        with pytest.raises(mg.ModgpuError, match="empty"):
            mg.readset_reset_bits(rs, 3, None)
        mg.readset_reset_bits(rs, 1, None)
        destroy(rs)
        # w > k: the last hit of a read lies less than w before its end
        reads = [(100, [(1, True, 10), (2, True, 75)]) for _ in range(3)]
        rs = build_set(str(tmp_path / "w"), 8, 30, 2, reads, [0, MS_RDNA | 1, MS_RDNA | 1])
        mg.readset_ref_flag_hits(rs, *hits, None)
        r = restatement_of(rs); r.ref_flag_hits(*hits)
        with pytest.raises(Refused):
            r.test_mods(1, 100)
        with pytest.raises(mg.ModgpuError, match="len - x - w"):
            mg.readset_test_mods(rs, 1, 100, None)
        destroy(rs)
        # two tested mods in reads of more than 20000 bases, and one: the reference clears 20000 cells between tested mods
        far = [(30000, [(1, True, 100), (2, True, 100)]), (30000, [(1, True, 100), (2, True, 100)])]
        for n_ok, want in ((2, "20000"), (1, None)):
            rs = build_set(str(tmp_path / ("f%d" % n_ok)), 19, 8, 2, far, [0, MS_RDNA | 1, MS_RDNA | (1 if n_ok == 2 else 0)])
            mg.readset_ref_flag_hits(rs, *hits, None)
            if want:
                r = restatement_of(rs)
                with pytest.raises(Refused):
                    r.test_mods(1, 100)
                with pytest.raises(mg.ModgpuError, match=want):
                    mg.readset_test_mods(rs, 1, 100, None)
            else:
                run_both(rs, ["-T", "1", "100"], str(tmp_path), hits)
            destroy(rs)
        # w > k: a partner further away than any read extends: xmin beyond the end array's extent (modasm.c:664 asserts)
        reads = [(100, [(1, True, 5), (2, True, 75)]), (200, [(2, True, 50)])]
        rs = build_set(str(tmp_path / "x"), 8, 30, 2, reads, [0, MS_RDNA | 1, MS_RDNA | 1])
        mg.readset_ref_flag_hits(rs, *hits, None)
        r = restatement_of(rs); r.ref_flag_hits(*hits)
        with pytest.raises(Refused):
            r.test_mods(1, 2)
        with pytest.raises(mg.ModgpuError, match="beyond"):
            mg.readset_test_mods(rs, 1, 2, None)
        destroy(rs)


def test_names_in_header_library_and_binding():
    header = open(os.path.join(util.ROOT, "include", "modgpu.h")).read()
    L = mg.lib()
    for n in NAMES:
        assert re.search(r"^int  %s \(" % n, header, re.M), n
    for n in HOOKS:
        assert re.search(r"^void %s \(" % n, header, re.M), n
    assert re.search(r"^const MgModInfo \*mgReadsetModInfo \(", header, re.M) and re.search(r"^const U8 \*mgReadsetReadFlags \(", header, re.M)
    for n in NAMES + HOOKS + ["mgReadsetModInfo", "mgReadsetReadFlags"]:
        assert n in mg.EXPORTS and hasattr(L, n), n
    assert [f[0] for f in mg.MgReadset._fields_][-2:] == ["bad", "contained"]          # the struct has no new field
    for f in ("readset_ref_flag", "readset_ref_flag_hits", "readset_reset_bits", "readset_test_mods", "readset_mod_info", "readset_read_flags", "readset_rdna_diag", "readset_rdna_grid"):
        assert callable(getattr(mg, f)), f


DESIGNED = ["A", "B", "C", "D", "E513", "E256", "E257", "F"]


@pytest.mark.parametrize("name", DESIGNED)
def test_designed_sets_through_the_host_loops(name, tmp_path):
    """the sets of tests/rdna_designs.py -- A three tiles of partners, B 1030 tested mods, C more than 256 partners, D i's first occurrence at the block
    lines, E count arrays of exactly 256, 257 and 513 cells, F positions across dx = 65535 -- each not refused and with its properties asserted from
    the restatement, then by rdnaTestModsHost: lines, YY, ZZ and state against the restatement, with and without the ZZ lines"""
    from tests import rdna_designs as rd
    assert sorted(DESIGNED) == sorted(rd.BUILDERS)
    with host_loops():
        for want_z in (True, False):
            rs = rd.load(name, tmp_path)
            r, diag, grid = rd.compare(name, rs, tmp_path, 1, want_z)
            assert diag[0] == 1 and grid == (0, 0, 0, 0)              # nothing was launched
            destroy(rs)
