"""Read sets built by design for the overlap passes (modasm -o1 / -o2 / -b / -c), shared by the CPU leg (tests/test_readset_overlap.py: the oracle
writes them, the library loads them, the host loops run) and the GPU leg (tests/test_gpu_readset_overlap.py: the device ingests them, the kernels of
mg_overlap.hip run), so that the two legs cannot drift.  A set is a list of reads made of pieces of tgc.world (8)'s genome; every property a set is
built for is asserted by its check_<set> from the restatement's records (tro.Restatement: per pair the matches (j, ihx)) or from the arrays, never
assumed -- a glued read can hold a k-mer of the genome across a joint, the genome holds a mod that is not copy 1.  A design that a seed does not
meet fails with a message that says which; nothing skips."""
import numpy as np

import modimizer_amd as mg
from tests import util
from tests import test_readset as trs
from tests import test_readset_overlap as tro
from tests import test_gpu_readset_clean as tgc

W = 8
K = tgc.K
SORT_TILE = tgc.SORT_TILE          # MG_RSORT_TILE (tests/test_abi.py holds it to the header)
SCAN_TILE = 4096
LDS_DEFAULT, LDS_MAX = 1024, 2048  # MG_OV_LDS_DEFAULT, MG_OV_LDS_MAX of mg_overlap.hip, as DESIGN.md documents them
TOPMASK = tro.TOPMASK
X0, X1, OUT = 10_000, 16_000, 24_000   # set A's query x = g[X0:X1]; g[OUT:] is the region x does not cover
cat = np.concatenate
rc = tgc.rc


class Design:
    def __init__(self, name, R, edit=False, **more):
        self.name, self.reads, self.edit = name, R.reads, edit
        self.at = {k: v + 1 for k, v in R.at.items()}           # name -> read number (reads from 1)
        self.__dict__.update(more)

    def no(self, name):
        return self.at[name]


def flip_classes(info):
    """the info edit of set B, in place on a view of info[0 .. max]: the copy class of 45 % of the mods drawn anew, so about a third is not copy 1"""
    rng = np.random.default_rng(77)
    n = len(info) - 1
    flip = rng.random(n) < 0.45
    new = info[1:].copy()
    new[flip] = (new[flip] & 0xfc) | rng.integers(0, 4, int(flip.sum())).astype(np.uint8)
    info[1:] = new


_copy1 = {}


def copy1_table(read):
    """the table a query is going to have without an info edit: its distinct seeds that the genome holds once (depth 1: copy 1 by -s 1 2 3)"""
    if not _copy1:
        tgc.world(W)
        h = tgc._worlds[W, "seeds"][0]
        seeds, n = np.unique(h.scan(tgc.world(W)[0])[0], return_counts=True)
        _copy1["h"], _copy1["once"] = h, seeds[n == 1]
    return int(np.isin(np.unique(_copy1["h"].scan(read)[0]), _copy1["once"]).sum())


class Builder(tgc.Reads):
    def P(self, a, n):
        """the piece of the genome from a with exactly n seeds"""
        return self.g[a:self.end_with(a, n)]

    def T(self, a, n):
        """the slice of the genome from a whose table has exactly n entries"""
        b = self.end_with(a, n)
        while copy1_table(self.g[a:b]) < n:
            b += 1
        return self.g[a:b]

    def junk(self, n):
        return self.rng.integers(0, 4, n).astype(np.uint8)

    def shaped(self, shape, minus, name, base=X0 + 100):
        """a partner of x whose hits are, piece by piece, ('in', n): n hits of x, or ('out', n): n hits of the region x does not cover.  The in-pieces
        lie in x in the order of y (plus), or in the opposite order and reverse-complemented (minus): in both the matches are in order"""
        ins = [i for i, (w, _) in enumerate(shape) if w == "in"]
        slot = {i: s for s, i in enumerate(ins[::-1] if minus else ins)}
        out_at, pieces = OUT, []
        for i, (w, n) in enumerate(shape):
            if w == "in":
                p = self.P(base + 900 * slot[i], n)
            else:
                e = self.end_with(out_at, n); p = self.g[out_at:e]; out_at = e + 40
            pieces.append(rc(p) if minus else p)
        self.add(cat(pieces), name)


SHAPES = {"l6364": [("in", 1), ("out", 62), ("in", 2)],          # matches exactly at j = 0, 63, 64: lane 63 of one stride, lane 0 of the next
          "gap": [("in", 40), ("out", 100), ("in", 30)],         # strides 0 and 2, no match at j in 64 .. 127
          "late": [("out", 70), ("in", 50)],                     # the first match at j >= 64
          "last0": [("in", 65), ("out", 20)]}                    # the last match in lane 0 of the last, partial stride
SIZES = (3, 63, 64, 65, 127, 128, 129, 193)


def add_set_a(R):
    g, P = R.g, R.P
    R.cut(X0, X1, "x")
    for i, n in enumerate(SIZES):
        a = X0 + 150 + 520 * i
        R.add(P(a, n), "p%d" % n); R.add(rc(P(a, n)), "m%d" % n)
    R.add(P(X0 + 1000, 2), "p2")
    for name, shape in SHAPES.items():
        R.shaped(shape, False, name + "+"); R.shaped(shape, True, name + "-")
    a1, a2 = X0 + 300, X0 + 2400
    R.add(cat([P(a2, 64), P(a1, 40)]), "re+")                                  # the out-of-order match is j = 64: its previous match is the carry
    R.add(cat([rc(P(a1, 64)), rc(P(a2, 40))]), "re-")
    R.add(cat([P(a2, 30), P(OUT, 100), P(a1, 40)]), "regap+")                  # ... and the carry has crossed a stride without matches
    R.add(cat([rc(P(a1, 30)), P(OUT, 100), rc(P(a2, 40))]), "regap-")
    R.add(cat([P(a1, 40), rc(P(a2, 40))]), "half")                             # nPlus == nMinus
    R.add(cat([P(a1, 30), rc(P(a2, 50))]), "mostly-")                          # nMinus > nPlus > 0
    R.add(cat([P(a1, 40)] * 2), "tandem_y")
    R.add(cat([P(a2, 1)] * 3), "thrice1")                                      # one table entry matched three times: the run is 3, equal ihx
    R.add(cat([P(a1 + 700, 50)] * 2), "tandem_x")
    c0 = X0 + 1500; c1 = R.end_with(c0, 150)
    R.add(g[c0:c1], "c")                                                       # the query of the contained / overlap decisions
    R.add(g[c0 - 1:c1], "c_eq")                 # firstDiff -1, len[x] - lastDiff == len[y]: contained
    R.add(g[c0:c1 + 400], "c_first0")           # firstDiff 0: overlap
    R.add(g[c0 + 1:c1 + 300], "c_first+")       # firstDiff +1: overlap
    R.add(g[c0 - 1:c1 - 1], "c_end1")           # firstDiff -1, len[x] - lastDiff == len[y] + 1: overlap
    R.add(g[c0 - 300:c1 + 300], "c_big")        # firstDiff < 0, len[x] - lastDiff < len[y]: contained


def set_a():
    R = Builder(W, 11)
    add_set_a(R)
    return Design("A", R)


def set_b():
    R = Builder(W, 12)
    add_set_a(R)
    R.add(np.zeros(0, np.uint8), "empty")
    for i in range(60):
        a = int(R.rng.integers(500, 37_000)); R.cut(a, a + int(R.rng.integers(1200, 1800)), flip=bool(i % 2))
    return Design("B", R, edit=True)


TABLES = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)


def set_c():
    R = Builder(W, 13)
    for i, n in enumerate(TABLES):
        R.add(R.T(1000 + 211 * i, n), "t%d" % n)
    R.cut(900, 22_000, "tbig")
    for i in range(8):
        R.cut(1200 + 2400 * i, 1200 + 2400 * i + 500 + 40 * i, "f%d" % i, flip=bool(i % 2))      # partners, and fillers of the query list
    return Design("C", R)


D_WIN, D_SAME = 5000, 70


def set_d():
    R = Builder(W, 14)
    for i in range(D_SAME):                                                     # the same slice, both strands: equal nHit in every list
        R.cut(D_WIN + 100, D_WIN + 1100, flip=bool(i % 2))
    for i in range(40):
        a = D_WIN + int(R.rng.integers(0, 200)); R.cut(a, a + int(R.rng.integers(950, 1050)), flip=bool(i % 2))
    for i in range(3):
        R.cut(D_WIN - 1500 * (i + 1), D_WIN + 1200 + 1000 * i, "long%d" % i)
    R.cut(30_000, 30_300, "loner")                                              # its only partner is itself: one pair
    return Design("D", R)


def set_e():
    R = Builder(W, 15)
    g = R.g
    R.add(cat([g[3000:5000], R.junk(70_000), g[6000:8000]]), "wrap")            # dx across the junk is more than 65535: it wraps
    R.add(cat([g[2000:22_000], R.junk(65_536 - 20_000), g[24_000:38_000]]), "long")      # the second piece begins at position 65536
    R.cut(23_900, 26_000, "y_long")             # begins 100 bases before long's second piece
    R.cut(5900, 8100, "y_wrap")                 # reaches 100 bases past either end of wrap's second piece
    R.cut(2500, 4000); R.cut(20_000, 23_000); R.cut(30_000, 33_000, flip=True); R.cut(6500, 7500, flip=True); R.cut(36_000, 39_000)
    return Design("E", R, first_piece=g[3000:5000])


BUILDERS = {"A": set_a, "B": set_b, "C": set_c, "D": set_d, "E": set_e}
_designs, _oracle = {}, {}


def design(name):
    if name not in _designs:
        _designs[name] = BUILDERS[name]()
    return _designs[name]


def oracle_set(name, stem=None):
    """(arrays, info) of the design through the oracle (pyoracle.Readset.read over tgc.world's set, set B's info edited first); with `stem` it
    writes <stem>.mod and <stem>.readset for mgReadsetLoad"""
    if name in _oracle and stem is None:
        return _oracle[name]
    from oracle import pyoracle as orc
    D = design(name)
    h = orc.Hasher(K, W, 17); oms = orc.Modset(h, 20)
    oms.add_sequence(np.zeros(100, np.uint8)); oms.add_sequence(tgc.world(W)[0])
    oms.set_copy(1, 2, 3)
    if D.edit:
        flip_classes(np.ctypeslib.as_array(oms.p.contents.info, (oms.max + 1,)))
    ors = orc.Readset(oms); ors.read(D.reads)
    _oracle[name] = (ors.arrays(), oms.infos())
    assert int(oms.depths().max()) < 0xffff, "set %s: a depth saturated" % name
    if stem:
        oms.write_mod(stem + ".mod"); ors.write(stem + ".readset")
    ors.close(); oms.close()
    return _oracle[name]


def ingest(name, tmp_path):
    """the design ingested on the device: (ms, rs); its arrays are the oracle's (which holds dx and len of set E)"""
    D = design(name)
    L = mg.lib()
    if not D.edit:
        ms, rs = tgc.ingest(D.reads, W, tmp_path)
    else:
        p = str(tmp_path / "m.mod"); open(p, "wb").write(tgc.world(W)[2])
        with mg.CFile(p, "r") as f:
            ms = L.modsetRead(f)
        flip_classes(np.ctypeslib.as_array(ms.contents.info, (ms.contents.max + 1,)))
        L.mgModsetHostChanged(ms)
        rs = L.mgReadsetCreate(ms)
        bases, offs = util.concat_reads(D.reads)
        assert L.mgReadsetRead(rs, bases.ctypes.data, offs.ctypes.data, len(D.reads)) == 0
    a, info = oracle_set(name)
    trs.same(trs.lib_arrays(rs), a)
    assert np.array_equal(tro.ms_info(ms), info)
    return ms, rs


# ---- what the records say about a pair ----

def records(r, x):
    return {rec["iy"]: rec for rec in r.pure(x)[1]}


def js(rec):
    return [j for j, _ in rec["match"]]


def strides(rec):
    return sorted({j // 64 for j in js(rec)})


def out_of_order(rec, minus):
    """the places in the match list whose ihx is below (plus) or above (minus) the match before it"""
    m = rec["match"]
    return [i for i in range(1, len(m)) if (m[i][1] > m[i - 1][1] if minus else m[i][1] < m[i - 1][1])]


def diffs(r, x, rec, bits=None, pos=None):
    """(firstDiff, lastDiff) of the pair (x, rec's y): position in x minus position in y at the first and at the last match; with `bits` the
    positions as a sum kept in that many bits would give them; with `pos` from other positions than the arrays'"""
    pos = r.pos if pos is None else pos
    mask = (1 << bits) - 1 if bits else -1
    a0, b0 = r.hs[x - 1], r.hs[rec["iy"] - 1]
    d = [(pos[a0 + ihx - 1] & mask) - (pos[b0 + j] & mask) for j, ihx in (rec["match"][0], rec["match"][-1])]
    return d[0], d[1]


def contained(first, last, x_len, y_len):
    return first < 0 and not x_len - last > y_len


# ---- the checks: every property a set is built for, from the restatement ----

def check_a(D, r):
    a = r.a
    x = D.no("x")
    recs = records(r, x)
    n_of = lambda name: int(a["nHit"][D.no(name) - 1])
    for n in SIZES:                                                             # hit counts of exactly 3, 63, 64, 65, 127, 128, 129, 193; both strands
        for s in "pm":
            y = D.no("%s%d" % (s, n)); rec = recs.get(y)
            assert n_of("%s%d" % (s, n)) == n and rec and rec["nHit"] == n and js(rec) == list(range(n)), "set A: no partner of exactly %d hits, all matched" % n
            assert (rec["rawMinus"], rec["rawPlus"]) == ((n, 0) if s == "m" else (0, n)), "set A: %s%d is not all on one strand" % (s, n)
            assert not out_of_order(rec, s == "m")
    assert js(recs[D.no("p129")])[-1] == 128 and n_of("p129") % 64 == 1         # the last match is lane 0 of the last, partial stride
    for s, minus in (("+", False), ("-", True)):
        rec = recs[D.no("l6364" + s)]
        assert js(rec) == [0, 63, 64] and rec["nHit"] == 3, "set A: matches exactly at j = 63 and j = 64 plus one more: %r" % js(rec)
        rec = recs[D.no("gap" + s)]
        assert strides(rec) == [0, 2] and n_of("gap" + s) > 128, "set A: matches in strides 0 and 2 and none at j in 64 .. 127: %r" % strides(rec)
        rec = recs[D.no("late" + s)]
        assert js(rec)[0] >= 64, "set A: the first match at j >= 64"
        rec = recs[D.no("last0" + s)]
        assert js(rec)[-1] == 64 and 65 < n_of("last0" + s) < 128, "set A: the last match is lane 0 of the last, partial stride"
        for name in ("l6364", "gap", "late", "last0"):
            rec = recs[D.no(name + s)]
            assert not out_of_order(rec, minus) and (rec["rawPlus"] == 0) == minus and (rec["rawMinus"] == 0) == (not minus), "set A: %s%s is not in order on one strand" % (name, s)
            assert rec["nBadOrder"] == 0 and rec["isPlus"] == (not minus)
    # rearranged: nLess (plus) and nGreater (minus) from a match that is the first of its stride, so the previous match is the wave's carry
    for name, minus, gap in (("re+", False, False), ("re-", True, False), ("regap+", False, True), ("regap-", True, True)):
        rec = recs[D.no(name)]
        o = out_of_order(rec, minus)
        assert len(o) == 1 and rec["nBadOrder"] == 1 and (rec["rawPlus"] == 0) == minus and (rec["rawMinus"] == 0) == (not minus), "set A: %s has not one out-of-order match on one strand" % name
        j, before = rec["match"][o[0]][0], rec["match"][o[0] - 1][0]
        assert before // 64 < j // 64 and all(k // 64 != j // 64 or k >= j for k in js(rec)), "set A: the out-of-order match of %s is not the first match of its stride" % name
        if gap:
            assert j // 64 - before // 64 >= 2, "set A: no stride without matches before the out-of-order match of %s" % name
        else:
            assert j == 64 and before == 63
    rec = recs[D.no("half")]                                                    # a forward and a reverse piece, nPlus == nMinus, longer than 64 hits
    assert rec["rawPlus"] == rec["rawMinus"] == 40 and n_of("half") > 64 and (rec["isPlus"], rec["nPlus"], rec["nMinus"], rec["nBadOrder"], rec["nBadFlip"]) == (0, 40, 40, 0, 0)
    rec = recs[D.no("mostly-")]                                                 # nMinus > nPlus > 0: neither branch adjusts
    assert rec["rawMinus"] > rec["rawPlus"] > 0 and n_of("mostly-") > 64 and (rec["isPlus"], rec["nPlus"], rec["nMinus"], rec["nBadOrder"]) == (0, rec["rawPlus"], rec["rawMinus"], 0)
    assert out_of_order(rec, True) and out_of_order(rec, False)                 # both order tests would count here, and neither is reported
    rec = recs[D.no("tandem_y")]                                                # a tandem partner: every table entry matched twice
    assert sorted(i for _, i in rec["match"][:40]) == sorted(i for _, i in rec["match"][40:]) and rec["nHit"] == 80 and rec["nBadOrder"] == 1
    rec = recs[D.no("thrice1")]                                                 # the ihx of neighbours are equal
    assert len({i for _, i in rec["match"]}) == 1 and js(rec) == [0, 1, 2] and rec["nHit"] == 3 and rec["nBadOrder"] == 0
    tx = D.no("tandem_x")                                                       # a tandem query: the table takes the first occurrence, the rest are nRepeat
    assert r.pure(tx)[0] == 50 and r.table_size[tx] == 50 and n_of("tandem_x") == 100
    assert all(i <= 50 for rec in r.pure(tx)[1] for _, i in rec["match"])
    assert x in recs and recs[x]["nHit"] == r.table_size[x]                     # x itself as its own partner
    assert r.runs[x][D.no("p2")] == 2 and D.no("p2") not in recs, "set A: no partner sharing exactly 2 active mods with x (dropped)"
    assert r.runs[x][D.no("p3")] == 3 and D.no("p3") in recs, "set A: no partner sharing exactly 3 active mods with x (kept)"
    # contained / overlap with the first and the last match in different strides, on both sides of equality at either end
    c = D.no("c")
    crecs = records(r, c)
    c_len = int(a["len"][c - 1])
    want = {"c_eq": (lambda f: f == -1, lambda e: e == 0, 1), "c_first0": (lambda f: f == 0, lambda e: e < 0, 0), "c_first+": (lambda f: f == 1, lambda e: e < 0, 0),
            "c_end1": (lambda f: f == -1, lambda e: e == 1, 0), "c_big": (lambda f: f < -1, lambda e: e < 0, 1)}
    for name, (first_ok, end_ok, is_con) in want.items():
        y = D.no(name); rec = crecs[y]
        first, last = diffs(r, c, rec)
        end = c_len - last - int(a["len"][y - 1])                               # > 0: x reaches past y's end
        assert len(strides(rec)) >= 2 and rec["isPlus"], "set A: %s: first and last match in one stride" % name
        assert first_ok(first) and end_ok(end), "set A: %s lands on the wrong side: firstDiff %d, len[x] - lastDiff - len[y] %d" % (name, first, end)
        assert rec["isContained"] == is_con == contained(first, last, c_len, int(a["len"][y - 1]))


def copy1_mask(a, info):
    return (info[a["hit"] & TOPMASK] & 3) == 1


def check_b(D, r):
    a, info = r.a, np.asarray(r.info)
    one = copy1_mask(a, info)
    share = 1 - one.mean()
    assert one.sum() > SCAN_TILE, "set B: the copy-1 hits (%d) do not exceed one scan tile" % one.sum()
    assert 0.25 < share < 0.45, "set B: %.2f of the hits are not copy 1, not about a third" % share
    hs = a["hitStart"].astype(np.int64)
    mixed = 0
    for i in range(len(a["nHit"])):                                              # a non-copy-1 hit before, between and after its copy-1 hits
        o = one[hs[i]:hs[i + 1]]
        at = np.flatnonzero(o)
        if len(at) >= 2 and not o[0] and not o[-1] and not o[at[0]:at[-1]].all():
            mixed += 1
    assert mixed, "set B: no query with a non-copy-1 hit before, between and after its copy-1 hits"
    x = D.no("x")
    assert r.pure(x)[1] and r.table_size[x] < int(a["nHit"][x - 1]) - 100       # the table's j + 1 are no longer 1, 2, 3, ..


def bounds(a, info, queries):
    """bound[] as ovlDrive defines it: per query the lengths of the inverse lists of its copy-1 hits, a repeat's list counted too"""
    hs, inv = a["hitStart"].astype(np.int64), a["invStart"].astype(np.int64)
    out = []
    for x in queries:
        m = (a["hit"][hs[x - 1]:hs[x]] & TOPMASK).astype(np.int64)
        m = m[(np.asarray(info)[m] & 3) == 1]
        out.append(int((inv[m + 1] - inv[m]).sum()))
    return out


def batch_sizes(bound, budget):
    """the batches ovlDrive cuts: a query joins while the batch's bounds stay within the budget; a batch holds at least one query"""
    out, q0 = [], 0
    while q0 < len(bound):
        q1, c = q0, 0
        while q1 < len(bound) and (q1 == q0 or c + bound[q1] <= budget):
            c += bound[q1]; q1 += 1
        out.append(q1 - q0); q0 = q1
    return out


def batch_queries(D, r, m=10):
    """set B's query list for the batch tests: m reads with candidates, then the read without hits, then the others; and the sum of the first m bounds"""
    n = len(D.reads)
    empty = D.no("empty")
    rest = [x for x in range(1, n + 1) if x != empty]
    queries = rest[:m] + [empty] + rest[m:]
    b = bounds(r.a, r.info, queries)
    assert b[m] == 0 and all(v > 0 for v in b[:m]) and b[m + 1] > 0
    return queries, b, sum(b[:m])


def check_c(D, r):
    for n in TABLES:
        x = D.no("t%d" % n)
        r.pure(x)
        assert r.table_size[x] == n, "set C: no table of exactly %d entries (%d)" % (n, r.table_size[x])
        assert len(r.pure(x)[1]) >= 2, "set C: the query of table %d has no partner" % n
    big = D.no("tbig"); r.pure(big)
    assert r.table_size[big] > 2500 and len(r.pure(big)[1]) >= 2, "set C: no table of more than 2500 entries"


def pair_starts(r, queries):
    """the first pair of every query in the pair kernel's order (by query, then by partner), and the number of pairs"""
    s, at = [], 0
    for x in queries:
        s.append(at); at += len(r.pure(x)[1])
    return s, at


def queries_c(D, r):
    """set C's query list: around each cap (64, 1024, 2048) the table of cap entries and the one of cap + 1 are neighbours, ordered and padded with
    filler queries so that the last pair of the first and the first pair of the second are waves of one workgroup of four"""
    fillers = [D.no("f%d" % i) for i in range(8)]
    odd = [f for f in fillers if len(r.pure(f)[1]) % 4]
    assert odd, "set C: no filler query whose pairs are no multiple of 4"
    queries, n = [], 0
    for lo, hi in ((64, 65), (1024, 1025), (2048, 2049), (63, 1023), (2047, None)):
        if (n + len(r.pure(D.no("t%d" % lo))[1])) % 4 == 0:
            queries.append(odd[0]); n += len(r.pure(odd[0])[1])
        for t in (lo, hi):
            if t:
                queries.append(D.no("t%d" % t)); n += len(r.pure(queries[-1])[1])
    queries += [D.no("tbig")] + fillers
    return queries


def lds_cap(setting):
    """the cap of a pair's table in LDS under MODGPU_OVERLAP_LDS = setting, as mg_overlap.hip documents it"""
    return LDS_DEFAULT if setting is None or setting < 0 else min(setting, LDS_MAX)


def check_c_paths(D, r, queries, setting):
    """both paths are taken under this setting (HBM alone under 0), and around a cap inside the tables' range two pairs on either side of it fall
    into one workgroup"""
    cap = lds_cap(setting)
    starts, n_pairs = pair_starts(r, queries)
    size = [r.table_size[x] for x in queries]
    live = [s for s, x in zip(size, queries) if r.pure(x)[1]]
    in_lds, in_hbm = [s for s in live if s <= cap], [s for s in live if s > cap]
    assert in_hbm and (in_lds or cap == 0), "set C: cap %d does not split the tables" % cap
    if cap == 0:
        assert not in_lds
        return
    assert cap in size and cap + 1 in size, "set C: no table of exactly cap and cap + 1 entries for cap %d" % cap
    q = size.index(cap)
    assert size[q + 1] == cap + 1
    last, first = starts[q + 1] - 1, starts[q + 1]
    assert starts[q] <= last and first < (starts[q + 2] if q + 2 < len(starts) else n_pairs)
    assert last // 4 == first // 4, "set C: the pairs on either side of cap %d are not in one workgroup of four" % cap


def check_d(D, r, tile=SORT_TILE):
    n = len(D.reads)
    queries = list(range(1, n + 1))
    starts, n_pairs = pair_starts(r, queries)
    assert n_pairs > tile, "set D: %d pairs do not exceed one sort tile" % n_pairs
    assert sum(r.cands[x] for x in queries) > 1_000_000
    found = False
    for x, s in zip(queries, starts):                                           # 20 entries of one nHit that lie on both sides of a tile line of the output
        recs = r.pure(x)[1]
        for i in range(len(recs)):
            k = i
            while k + 1 < len(recs) and recs[k + 1]["nHit"] == recs[i]["nHit"]:
                k += 1
            if k - i + 1 >= 20 and (s + i) // tile < (s + k) // tile:
                found = True
    assert found, "set D: no list with 20 entries of one nHit across a tile line"
    loner = D.no("loner")
    assert [rec["iy"] for rec in r.pure(loner)[1]] == [loner], "set D: the loner's only partner is not itself"


def subsets_d(D, r):
    """query lists with nPairs of 1 and of every residue of 4, small and large"""
    loner, big = D.no("loner"), 1
    nb = len(r.pure(big)[1])
    out = [[loner] * k for k in (1, 2, 3, 4)] + [[big] + [loner] * k for k in range(4)]
    res = {pair_starts(r, q)[1] % 4 for q in out if pair_starts(r, q)[1] > 4}
    assert pair_starts(r, out[0])[1] == 1 and res == {0, 1, 2, 3} and nb > 64
    return out


def check_e(D, r):
    a = r.a
    wrap, long_, y_long, y_wrap = (D.no(k) for k in ("wrap", "long", "y_long", "y_wrap"))
    hs = r.hs
    n1 = tgc.hits_of(W, D.first_piece)
    dx = a["dx"][hs[wrap - 1]:hs[wrap]].astype(np.int64)
    # the gap across the junk is 70000 and some bases of the pieces: the stored dx is that minus 65536
    assert n1 < len(dx) and 70_000 - 65_536 <= int(dx[n1]) < 70_000 - 65_536 + 200, "set E: dx across the junk did not wrap: %d" % int(dx[n1])
    assert int(a["len"][long_ - 1]) > 65_536 and int(a["len"][wrap - 1]) > 65_536
    pos_long = np.array(r.pos[hs[long_ - 1]:hs[long_]])
    assert (pos_long < 65_536).sum() > 1000 and (pos_long >= 65_536).sum() > 1000 and np.diff(pos_long).max() < 65_536, "set E: long's positions do not pass 2^16 with hits on both sides"
    for big, small in ((wrap, y_wrap), (long_, y_long)):                        # both are queries and partners of plain reads
        assert small in records(r, big) and big in records(r, small)
    # a 16-bit pos would decide otherwise: y_long lies in long (contained), but with positions kept in 16 bits its first match would come out ahead
    rec = records(r, y_long)[long_]
    xl, yl = int(a["len"][y_long - 1]), int(a["len"][long_ - 1])
    f, l = diffs(r, y_long, rec); f16, l16 = diffs(r, y_long, rec, bits=16)
    assert rec["isContained"] == 1 == contained(f, l, xl, yl) and not contained(f16, l16, xl, yl), "set E: a 16-bit pos decides (y_long, long) the same"
    # the wrapped dx decides (y_wrap, wrap): y_wrap reaches past wrap's end, yet wrap's positions are 65536 short, so the reference calls it contained
    rec = records(r, y_wrap)[wrap]
    xl, yl = int(a["len"][y_wrap - 1]), int(a["len"][wrap - 1])
    f, l = diffs(r, y_wrap, rec)
    true_pos = list(r.pos)
    for h in range(hs[wrap - 1] + n1, hs[wrap]):
        true_pos[h] += 65_536
    ft, lt = diffs(r, y_wrap, rec, pos=true_pos)
    assert rec["isContained"] == 1 == contained(f, l, xl, yl) and not contained(ft, lt, xl, yl), "set E: the decision on (y_wrap, wrap) does not depend on dx wrapping"
    flags = [rec["isContained"] for x in (wrap, long_) for rec in r.pure(x)[1]] + [records(r, x)[b]["isContained"] for x in range(1, r.n + 1) for b in (wrap, long_) if b in records(r, x)]
    assert 0 in flags and 1 in flags


CHECKS = {"A": check_a, "B": check_b, "C": check_c, "D": check_d, "E": check_e}
_checked = {}


def checked(name, a, info):
    """a restatement of the design on these arrays whose properties have been asserted; the pure records are shared by the tests of a module (they
    are never changed), the flags are each caller's: take fresh() of it"""
    if name not in _checked:
        r = tro.Restatement(a, info)
        CHECKS[name](design(name), r)
        _checked[name] = r
    return _checked[name]


def fresh(r0):
    """a restatement with r0's records and flags of its own"""
    for x in range(1, r0.n + 1):
        r0.pure(x)
    r = tro.Restatement.__new__(tro.Restatement)
    r.__dict__.update(r0.__dict__)
    r.bad, r.contained, r.out = [0] * (r0.n + 1), [0] * (r0.n + 1), []
    return r


CMDS = ["-o2", "3", "-b", "-c", "-o2", "1", "-o1", "1", "-b", "-c"]


def compare(rs, r, queries, tmp_path, path, cmds=CMDS):
    """the lists of `queries` in one call, then the command sequence, through the library against the restatement r (flags zero on both sides):
    lists, lines, flags, the diag totals.  `path`: 0 the device, 1 the host loops"""
    L = mg.lib()
    want = [r.find_overlaps(x, 0) for x in queries]
    got = mg.readset_find_overlaps(rs, queries, 0, None, want_lists=True)
    assert L.mgReadsetOverlapsPath() == path
    assert got == want
    assert tro.lib_flags(rs)[0] == r.bad
    d = mg.readset_overlaps_diag()
    assert d[1:3] == (sum(r.cands[x] for x in queries), sum(len(r.pure(x)[1]) for x in queries)), d
    before = len(r.out)
    text = tro.lib_run(rs, cmds, str(tmp_path / "lines.txt"))
    assert L.mgReadsetOverlapsPath() == path
    r.run(cmds)
    assert text == "".join(r.out[before:])
    assert tro.lib_flags(rs) == (r.bad, r.contained)
    return d, got


def reset(rs):
    """the reads' bad flags back to zero, as a fresh restatement has them"""
    for i in range(rs.contents.nReads + 1):
        rs.contents.bad[i] = 0


def lists(rs, r0, queries, path):
    """the lists of `queries` from zeroed flags, held against the restatement; returns (lists, diag)"""
    reset(rs)
    r = fresh(r0)
    want = [r.find_overlaps(x, 0) for x in queries]
    got = mg.readset_find_overlaps(rs, queries, 0, None, want_lists=True)
    assert mg.lib().mgReadsetOverlapsPath() == path
    assert got == want and tro.lib_flags(rs)[0] == r.bad
    d = mg.readset_overlaps_diag()
    assert d[1:3] == (sum(r.cands[x] for x in queries), pair_starts(r, queries)[1]), d
    return got, d


def batches_b(rs, r0, path, m=10):
    """set B under MODGPU_OVERLAP_CANDS exactly the sum of the bounds of the first m queries, and that minus one: the batch count exactly, the query
    without candidates joining the batch before it, the results of the one-batch run"""
    D = design("B")
    queries, b, budget = batch_queries(D, r0, m)
    one, d = lists(rs, r0, queries, path)
    assert d[0] == 1
    for bud, first in ((budget, m + 1), (budget - 1, m - 1)):
        sizes = batch_sizes(b, bud)
        assert sizes[0] == first and len(sizes) > 2                             # exact: the m queries and the one without candidates; one less: m - 1
        if bud == budget - 1:
            assert sizes[1] >= 2                                                # here it joins the batch that query m opens
        with mg.knobs(OVERLAP_CANDS=bud):
            got, d = lists(rs, r0, queries, path)
        assert d[0] == len(sizes), "OVERLAP_CANDS %d: %d batches, not %d" % (bud, d[0], len(sizes))
        assert got == one
        at, with_pairs = 0, 0
        for n in sizes:                                                         # the pair kernel is launched once per batch that has a pair
            with_pairs += any(r0.pure(x)[1] for x in queries[at:at + n]); at += n
        assert d[3] == (0 if path else with_pairs)


def many_pairs_d(rs, r0, path):
    """set D's subsets (nPairs 1, every residue of 4) and a query list of more than 1024 with every read many times"""
    D = design("D")
    for q in subsets_d(D, r0):
        lists(rs, r0, q, path)
    unit = list(range(D_SAME + 1, D_SAME + 41)) + [D.no("loner")]
    queries = unit * (1024 // len(unit) + 1)
    assert len(queries) > 1024
    got, d = lists(rs, r0, queries, path)
    assert d[0] == 1 and not any(tro.lib_flags(rs)[0])
    for i in range(len(unit), len(queries)):                                    # each copy gets the same records
        assert got[i] == got[i - len(unit)]


LDS_SETTINGS = (64, None, 2048, 4096, 0, -1)


def tables_c(rs, r0, path):
    """set C's query list under every MODGPU_OVERLAP_LDS: both paths in each launch (HBM alone under 0), identical results"""
    D = design("C")
    queries = queries_c(D, r0)
    seen = []
    for setting in LDS_SETTINGS:
        check_c_paths(D, r0, queries, setting)
        with mg.knobs(OVERLAP_LDS=setting):
            got, d = lists(rs, r0, queries, path)
        assert d[0] == 1 and (path or d[3] == 1)
        seen.append(got)
    assert all(s == seen[0] for s in seen)


EXTRAS = {"B": batches_b, "C": tables_c, "D": many_pairs_d}


# (query, partner) whose record a set is built for: the replay must not hide it behind a skip (a partner that an earlier query marked bad)
SHOWN = {"A": [("x", n) for n in ["%s%d" % (s, k) for s in "pm" for k in SIZES] + [k + s for k in SHAPES for s in "+-"]
               + ["re+", "re-", "regap+", "regap-", "half", "mostly-", "tandem_y", "thrice1"]]
              + [("c", n) for n in ("c_eq", "c_first0", "c_first+", "c_end1", "c_big")],
         "E": [("y_long", "long"), ("y_wrap", "wrap"), ("long", "y_long"), ("wrap", "y_wrap")]}


def queries_of(name, r0):
    """the query list of a set's main call: every read (set C: queries_c), in set E the plain reads before the two long ones"""
    D = design(name)
    if name == "C":
        return queries_c(D, r0)
    q = list(range(1, len(D.reads) + 1))
    if name == "E":
        last = [D.no("long"), D.no("wrap")]
        q = [x for x in q if x not in last] + last
    return q


def run_set(name, rs, r0, tmp_path, path):
    """everything a leg does with a designed set once it holds it: every read's list in one call and the command sequence (compare), then the set's
    own cases"""
    D = design(name)
    queries = queries_of(name, r0)
    d, got = compare(rs, fresh(r0), queries, tmp_path, path)
    assert d[0] == 1 and d[3] == (0 if path else 1)
    for qn, yn in SHOWN.get(name, ()):
        e = [e for e in got[queries.index(D.no(qn))] if e[0] == D.no(yn)]
        assert len(e) == 1 and not e[0][4] & tro.F_SKIPPED, "set %s: the record of (%s, %s) is hidden by a skip" % (name, qn, yn)
    if name in EXTRAS:
        EXTRAS[name](rs, r0, path)
