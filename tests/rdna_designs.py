"""Read sets built by design for the -T kernels of mg_rdna.hip, shared by the CPU leg (tests/test_readset_rdna.py: the host loops) and the GPU leg
(tests/test_gpu_readset_rdna.py: the kernels), so that the two legs cannot drift.  A set is made by test_readset_rdna.build_set from lists of
(mod, forward, dx); entry 0 fails checkMod and every mod 1 .. n_mods passes it, so mod j has partner ordinal j - 1 and nP = n_mods.  A filler mod sits
in few reads and the tested mods in more, so the depth range of the -T picks exactly the tested mods.  A read is as long as its last hit's position
plus w plus a tail: no visit counts before its array and no distance is looked up beyond it.  Every property a set is built for is asserted by its
check_<set> from the restatement's records of the -T (Rdna.tested / ext / start_cells / end_cells / cell_mods / first), never assumed, before the
library is compared; a design that is refused fails."""
import os

import numpy as np

import modimizer_amd as mg
from tests import test_readset_rdna as trd

K, W = 19, 8
OK = trd.MS_RDNA | 1                                                  # passes checkMod
TILE = 4096                                                           # MG_RD_TILE of mg_rdna.hip, as DESIGN.md documents it


class Design:
    def __init__(self, name, n_mods, reads, lo, hi, tested, **more):
        self.name, self.n_mods, self.reads, self.lo, self.hi, self.tested = name, n_mods, reads, lo, hi, tested
        self.info = [0] + [OK] * n_mods
        self.hits = (np.array([n_mods], np.uint32), np.array([5], np.int32))      # the reference sequence's one hit: the last mod
        self.cmds = ["-R", "x", "-T", str(lo), str(hi)]
        self.__dict__.update(more)


def read(hits, tail=3):
    """(length, hits) of hits = [(mod, forward, dx), ...]: the last hit's position + w + tail"""
    return (sum(h[2] for h in hits) + W + tail, list(hits))


def dx_of(j):
    return 1 + j % 4


def run_of(mods, skip=()):
    """the mods in order, strands alternating, dx 1 .. 4"""
    return [(m, j % 2 == 0, dx_of(j)) for j, m in enumerate(m for m in mods if m not in skip)]


# ---- A: three tiles of partner ordinals (mgRdnaAccumKernel: tile0 = blockIdx.y * MG_RD_TILE, o >= MG_RD_TILE, tile0 + o < nP; Emit and Rule beyond 256) ----

A_NP = 8197
A_A, A_B, A_C = 100, 200, 8195                                        # ordinals 99 and 199 (tile 0) and 8194 (tile 2)
A_ORDS = (0, 255, 256, 257, 511, 512, 4094, 4095, 4096, 4097, 8191, 8192, 8196)


def set_a():
    """nP = 8197: tiles of 4096, 4096 and 5 ordinals.  Tested: a = mod 100 in two reads of about 4100 hits that cross the tile lines (cells in every
    tile, at every ordinal of A_ORDS), partners 8192 and 8193 on both sides of it across the line between tiles 1 and 2 (split), ten visits that reach
    further than any partner (nBadLD of the single partners behind it in tiles 1 and 2); b = mod 200 with cells in tile 1 alone, at its first and last
    ordinal; c = mod 8195 in tile 2, twice in a read: a cell of itself"""
    big1 = run_of(range(1, 4099), skip=(A_B,))                        # ordinals 0 .. 4097, a at hit 99, forward
    assert big1[99] == (A_A, False, dx_of(99))
    big1[99] = (A_A, True, dx_of(99))
    big2 = run_of(range(4095, A_NP + 1))                              # ordinals 4094 .. 8196, a put in at hit 2000, reverse
    big2.insert(2000, (A_A, False, 2))
    reads = [read(big1), read(big2),
             read([(A_A, True, 9), (8192, True, 3), (8193, False, 2)]),              # behind a here, before it (a reverse) in big2
             read([(4096, True, 4), (A_A, True, 7)]), read([(A_A, True, 6), (4097, False, 5)]), read([(A_A, False, 11)])]
    reads += [read([(A_A, True, 6000)], tail=k) for k in range(10)]
    reads += [read([(4097, True, 3), (A_B, True, 8), (8192, False, 6)])] + [read([(A_B, k % 2 == 0, 5 + k), (5000 + k, True, 4)]) for k in range(4)]
    reads += [read([(A_C, True, 7), (1, True, 3), (A_C, False, 4), (4098, True, 2)]), read([(5, True, 2), (A_C, False, 9)]), read([(A_C, True, 4)])]
    return Design("A", A_NP, reads, 5, 100, [A_A, A_B, A_C])


def check_a(D, r):
    assert r.tested == D.tested and r.m - 1 == A_NP and A_NP % 256 and A_NP % TILE and (A_NP + TILE - 1) // TILE == 3 and A_NP - 2 * TILE == 5
    ords = {i: {m - 1 for m in r.cell_mods[i]} for i in r.tested}
    assert set(A_ORDS) <= ords[A_A], "set A: a's cells miss ordinals %r" % sorted(set(A_ORDS) - ords[A_A])
    assert all(any(o // TILE == t for o in ords[A_A]) for t in range(3))
    assert ords[A_B] and min(ords[A_B]) == TILE and max(ords[A_B]) == 2 * TILE - 1, "set A: b's cells are not in tile 1 alone, at its first and last ordinal"
    assert (A_C - 1) // TILE == 2 and A_C - 1 in ords[A_C], "set A: c is not a cell of itself"
    assert {o // TILE for o in ords[A_C]} == {0, 1, 2}
    assert any(r.first[A_C].count(v) == 2 for v in r.first[A_C])      # the read that holds c twice is visited twice
    assert r.mi[A_A][5] >= 2 and r.mi[8192][6] == 1 and r.mi[8193][6] == 1, "set A: no split across the line between tiles 1 and 2"      # nSplit of a, nSplitLD
    bad = [m for m in range(1, A_NP + 1) if r.mi[m][4] and m not in D.tested]
    assert any((m - 1) // TILE == 1 for m in bad) and any((m - 1) // TILE == 2 for m in bad), "set A: no nBadLD of another mod in tiles 1 and 2"
    assert max(max(e) for e in r.ext.values()) <= 20000 and max(len(h) for _, h in D.reads) > TILE


# ---- B: the share of the visits (mgRdnaTestModsDevice: while (share < 16 && n * nTiles * share < 1024)) ----

B_MODS, B_DEEP = 1030, 7
B_BATCHES = ((1024, 1), (512, 2), (511, 4), (256, 4), (128, 8), (127, 16))      # MODGPU_TESTMODS_BATCH, the least share of the call


def set_b():
    """1030 mods, all tested, in one tile: five times every mod once, in reads of 40 hits, so with share 1 (a batch of 1024) two of a workgroup's four
    waves walk a second visit; mod 7 in 40 reads more"""
    rng = np.random.default_rng(23)
    reads = []
    for _ in range(5):
        p = rng.permutation(np.arange(1, B_MODS + 1))
        for a in range(0, B_MODS, 40):
            reads.append([(int(m), bool(rng.integers(0, 2)), int(rng.integers(0, 30))) for m in p[a:a + 40]])
    for k in range(40):
        hits = reads[k]
        j = int(rng.integers(0, len(hits)))
        if all(h[0] != B_DEEP for h in hits):
            hits[j] = (B_DEEP,) + hits[j][1:]
    reads = [read(h, tail=int(rng.integers(0, 20))) for h in reads]
    return Design("B", B_MODS, reads, 1, 200, list(range(1, B_MODS + 1)))


def check_b(D, r):
    assert r.tested == D.tested and len(r.tested) >= 1030 and r.m - 1 <= TILE
    assert r.depth[B_DEEP] >= 40 and sum(1 for i in r.tested if r.depth[i] >= 5) > 900
    assert 50_000 < sum(len(c) for c in r.cell_mods.values()) < 400_000
    for batch, share in B_BATCHES:                                    # the formula, for the record: the tests read the shares from mgReadsetRdnaGrid
        sizes = [min(batch, B_MODS - t) for t in range(0, B_MODS, batch)]
        assert sizes[-1] < sizes[0] and len(sizes) == batches_b(batch)


def batches_b(batch):
    return (B_MODS + batch - 1) // batch


# ---- C: more than 256 partners on one tile (mgRdnaRuleKernel: o += 256; mgRdnaEmitKernel: base += 256, at += tot) ----

C_NP, C_ONE, C_ALL = 600, 300, 514
C_ORDS = (0, 254, 255, 256, 257, 511, 512, 513, 599)


def set_c():
    """nP = 600.  Mod 300 has cells at the ordinals C_ORDS alone, none in [258, 510]; mod 514 (ordinal 513, the only read they share holds the two alone)
    has a cell at every ordinal, its own among them"""
    mods = [o + 1 for o in C_ORDS if o + 1 != C_ALL]
    reads = [read([(C_ALL, True, 4), (C_ONE, False, 9)]),
             read(run_of(mods[:4]) + [(C_ONE, True, 3)] + run_of(mods[4:])), read([(C_ONE, False, 2)]),
             read(run_of(range(1, C_NP + 1), skip=(C_ONE,)) + [(C_ALL, False, 3)]), read([(C_ALL, True, 1)])]
    return Design("C", C_NP, reads, 3, 100, [C_ONE, C_ALL])


def check_c(D, r):
    assert r.tested == D.tested and r.m - 1 == C_NP
    assert [m - 1 for m in r.cell_mods[C_ONE]] == list(C_ORDS) and not any(258 <= m - 1 <= 510 for m in r.cell_mods[C_ONE])
    assert r.cell_mods[C_ALL] == list(range(1, C_NP + 1))


def zz_order(zz):
    """(i, m) of the ZZ lines, in their order"""
    return [(int(l.split()[1]), int(l.split()[5])) for l in zz.splitlines()]


# ---- D: the first occurrence of i (mgRdnaVisitKernel: the ballot over 64 hits, __ffsll, break) ----

D_I = 1
D_FIRST = (0, 63, 64, 65, 127, 128)
D_LAST = (64, 65, 129, 200)
D_TWICE = ((10, 150), (70, 130), (5, 40), (70, 100), (63, 64), (128, 199))      # blocks 0 and 2, 1 and 2, twice in block 0, twice in block 1, across a line, the last hit


class Fill:
    """filler mods, each used once"""
    def __init__(self, first):
        self.next = first

    def run(self, n, at=()):
        """n hits of fresh mods, `at`: {hit number: (mod, forward)} put in their place"""
        out = []
        for j in range(n):
            if j in at:
                out.append(at[j] + (dx_of(j),))
            else:
                out.append((self.next, j % 3 != 0, dx_of(j))); self.next += 1
        return out


def set_d():
    """i = mod 1, alone tested.  Reads of 200 hits with i first at hit 0, 63, 64, 65, 127, 128; reads of 64, 65, 129 and 200 hits with i as the last
    hit; i twice, on opposite strands and at different positions: in blocks 0 and 2, 1 and 2, twice in one block of 64, on both sides of a block line
    (each such read is in inv[i] twice and is visited twice from the first occurrence); both strands"""
    F = Fill(2)
    reads = []
    for k, p in enumerate(D_FIRST):
        reads.append(read(F.run(200, {p: (D_I, k % 2 == 0)})))
    for k, n in enumerate(D_LAST):
        reads.append(read(F.run(n, {n - 1: (D_I, k % 2 == 1)})))
    for k, (p, q) in enumerate(D_TWICE):
        reads.append(read(F.run(200, {p: (D_I, k % 2 == 0), q: (D_I, k % 2 == 1)})))
    return Design("D", F.next, reads, 3, 100, [D_I], first_read_twice=len(D_FIRST) + len(D_LAST) + 1)


def check_d(D, r):
    assert r.tested == [D_I]
    first = r.first[D_I]                                              # (read, hit number, forward) per visit, by read
    want = list(D_FIRST) + [n - 1 for n in D_LAST] + [p for p, _ in D_TWICE for _ in range(2)]
    assert [f for _, f, _ in first] == want, "set D: i's first occurrences are at %r" % [f for _, f, _ in first]
    assert [r.a["nHit"][rd - 1] for rd, _, _ in first[len(D_FIRST):len(D_FIRST) + len(D_LAST)]] == list(D_LAST)
    assert {fw for _, _, fw in first} == {True, False}
    for k, (p, q) in enumerate(D_TWICE):                              # the second occurrence: the other strand, another position; the read is visited twice
        rd = D.first_read_twice + k
        assert first[len(D_FIRST) + len(D_LAST) + 2 * k][0] == first[len(D_FIRST) + len(D_LAST) + 2 * k + 1][0] == rd
        h0 = r.hs[rd - 1]
        assert r.mod[h0 + p] == r.mod[h0 + q] == D_I and r.fwd[h0 + p] != r.fwd[h0 + q] and r.pos[h0 + p] != r.pos[h0 + q]
        assert D_I in r.cell_mods[D_I]
    assert any(p // 64 == q // 64 for p, q in D_TWICE) and any(p // 64 == 0 and q // 64 == 2 for p, q in D_TWICE)


# ---- E: the suffix sums' steps of 256 cells (mgRdnaSuffixKernel: top > 256 ? top - 256 : 0, carry += tot) ----

E_I = 1
E_CELLS = {"E513": (0, 255, 256, 511, 512), "E256": (0, 255), "E257": (0, 255, 256)}


def set_e(name):
    """i = mod 1, alone tested, forward in every read, so a visit's start cell is x and its end cell len - x - w.  The visits' start cells are exactly
    E_CELLS[name] and their end cells the same, the greatest start with the least end.  Before i in the visit with the greatest x, and behind it in
    the visit with the greatest end, single partners at every distance among 0, 255, 256, 257, 512 that the arrays hold: the ZZ line of each prints
    the suffix sum at that cell"""
    cells = E_CELLS[name]
    top = cells[-1]
    F = Fill(2)
    reads = []
    for s, e in zip(cells, cells[::-1]):
        before, behind = [], []
        if s == top:                                                  # partners at positions top - d, ascending; the one at distance 0 shares i's position
            at = 0
            for d in sorted((d for d in (0, 255, 256, 257, 512) if d <= top), reverse=True):
                before.append((F.next, d % 2 == 0, top - d - at)); F.next += 1; at = top - d
            hits = before + [(E_I, True, top - at)]
        else:
            hits = [(E_I, True, s)]
        if e == top:
            at = 0
            for d in sorted(d for d in (255, 256, 257, 512) if d <= top):
                behind.append((F.next, d % 2 == 0, d - at)); F.next += 1; at = d
            reads.append((s + W + e, hits + behind))
        else:
            reads.append((s + W + e, hits))
    return Design(name, F.next, reads, 2, 100, [E_I], top=top)


def check_e(D, r):
    cells = list(E_CELLS[D.name])
    assert r.tested == [E_I] and r.start_cells[E_I] == cells and r.end_cells[E_I] == cells and r.ext[E_I] == (D.top + 1, D.top + 1)
    steps = (D.top + 1 + 255) // 256
    assert steps == {"E513": 3, "E256": 1, "E257": 2}[D.name]
    looked = {"-": set(), "+": set()}
    for l in r.zz[str(r.run_no)].splitlines():
        t = l.split()
        looked[t[8]] |= {int(t[14]), int(t[18])}
    want = {d for d in (0, 255, 256, 257, 512) if d <= D.top}
    assert looked["-"] == want and looked["+"] == want - {0}, "set %s: the rules look at %r" % (D.name, looked)


# ---- F: positions (mgRdnaPosKernel: the carry across 64 hits) ----

F_I = 1
F_READS = (64, 65, 128, 129)
F_BIG = (63, 64, 127)


def set_f():
    """i = mod 1, alone tested: the last hit (reverse in the third, else forward) of reads of 64, 65, 128 and 129 hits whose dx is 65535 at hits 63, 64 and 127 and small
    elsewhere, and the first hit, reverse, of one more of 129 hits: x and every distance pass through the carry.  Its count arrays pass 20000 cells:
    it is the only tested mod"""
    F = Fill(2)
    reads = []
    for n in F_READS + (129,):
        at = {n - 1: (F_I, n != 128)} if len(reads) < len(F_READS) else {0: (F_I, False)}
        hits = [(m, fw, 65535 if j in F_BIG else dx) for j, (m, fw, dx) in enumerate(F.run(n, at))]
        reads.append(read(hits))
    return Design("F", F.next, reads, 2, 100, [F_I])


def check_f(D, r):
    assert r.tested == [F_I]
    assert [int(r.a["nHit"][rd - 1]) for rd, _, _ in r.first[F_I]] == list(F_READS) + [129]
    assert [f for _, f, _ in r.first[F_I]] == [n - 1 for n in F_READS] + [0]
    dx = np.asarray(r.a["dx"], np.int64)
    for rd, _, _ in r.first[F_I]:
        n = int(r.a["nHit"][rd - 1])
        d = dx[r.hs[rd - 1]:r.hs[rd]]
        assert [j for j in range(n) if d[j] == 65535] == [j for j in F_BIG if j < n] and d[d != 65535].max() <= 4
    assert max(r.start_cells[F_I]) > 3 * 65535 and max(r.end_cells[F_I]) > 3 * 65535 and min(r.ext[F_I]) > 20000
    far = [int(l.split()[18]) for l in r.zz[str(r.run_no)].splitlines()]
    assert max(far) > 3 * 65535 and any(65535 < v < 2 * 65535 for v in far) and any(v < 65535 for v in far)


BUILDERS = {"A": set_a, "B": set_b, "C": set_c, "D": set_d, "E513": lambda: set_e("E513"), "E256": lambda: set_e("E256"), "E257": lambda: set_e("E257"), "F": set_f}
CHECKS = {"A": check_a, "B": check_b, "C": check_c, "D": check_d, "E513": check_e, "E256": check_e, "E257": check_e, "F": check_f}
_designs, _checked = {}, {}


def design(name):
    if name not in _designs:
        _designs[name] = BUILDERS[name]()
    return _designs[name]


def load(name, tmp):
    """a fresh load of the design (a -T changes info[]: every call gets its own); the caller destroys it with test_readset_rdna.destroy"""
    D = design(name)
    d = os.path.join(str(tmp), "set%s_%d" % (name, len(os.listdir(str(tmp)))))
    os.mkdir(d)
    return trd.build_set(os.path.join(d, "s"), K, W, D.n_mods, D.reads, D.info)


def checked(name, rs):
    """the restatement after the design's -R and -T on this load, not refused, the design's properties asserted.  Made once per design and shared (the
    loads of a design are the same arrays); never changed"""
    if name not in _checked:
        D = design(name)
        r = trd.restatement_of(rs)
        refused = trd.restatement_run(r, D.cmds, lambda _f: D.hits)
        assert refused is None, "set %s is refused: %s" % (name, refused)
        assert [i for i in range(r.m) if trd.check_mod(D.info[i])] == list(range(1, D.n_mods + 1))      # mod j has partner ordinal j - 1
        assert sum(1 for e in r.ext.values() if max(e) > 20000) <= 1
        CHECKS[name](D, r)
        _checked[name] = r
    return _checked[name]


def compare(name, rs, tmp, path, want_z=True):
    """the design's -R and -T through the library on a fresh load against the checked restatement: lines, YY, ZZ (if wanted), state, the path taken and
    the Diag counts.  Returns (restatement, Diag, Grid)"""
    D = design(name)
    r = checked(name, rs)
    d = os.path.join(str(tmp), "run%d" % len(os.listdir(str(tmp))))
    os.mkdir(d)
    out, yy, zz, err = trd.lib_run(rs, D.cmds, d, lambda _f: D.hits, want_z)
    assert err is None, err
    assert mg.lib().mgReadsetRdnaPath() == path
    assert out == "".join(r.out) and yy == r.yy
    if want_z:
        assert zz == r.zz
        assert zz_order(zz["1"]) == sorted(zz_order(zz["1"])) and len(zz["1"].splitlines()) == sum(len(c) for c in r.cell_mods.values())
    else:
        assert zz == {"1": ""}
    trd.same_state(rs, r)
    diag, grid = mg.readset_rdna_diag(), mg.readset_rdna_grid()
    assert diag[1:] == r.diag
    return r, diag, grid
