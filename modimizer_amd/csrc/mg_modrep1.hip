/* mg_modrep1.hip — modrep -s1 and -s2 on the device (modrep.c:272-489, 493-539).
 *
 * -s1's per-read pass is mg_modrep.hip's (vote, orient, hits).  This file is the END of the file: the state is the hits (k, x, read) in
 * (read, position) order with the reads' starts, n[k], and one persistent (k, n, x) per mod for pre[0].  Every stage is a few kernels
 * over hits, links, entries or mods; the host prints a line between them and sorts the report.
 *
 *   compaction   flags, the shared exclusive scan, an ordered scatter, the reads' new starts (counts by atomics, scanned).
 *   run removal  a wave per read, its positions 64 at a time in registers: ballot picks the next kept hit, a shuffle hands on its x.
 *   buildPrePost the links (k0, k1, dx) of neighbouring hits, in hit order: their ordinal is their arrival time.  Per side (post: owner
 *                k0, partner k1; pre: owner k1, partner k0) the ordinals are sorted stably by partner, then by owner (mgRefStableSort
 *                twice).  A run of equal (owner, partner) is an entry; a link's rank in its run is c, its occurrence number.
 *   addHit order modrep.c:129-148 moves an entry to the front when its count passes the front's, so the front holds M, the largest c so
 *                far in the list.  An arrival with c > M is a record; M grows by one at a time, so the record of value v is the FIRST
 *                arrival of the owner with c == v: atomicMin of the ordinal into slot (owner's first link + v - 1).  The list is: the
 *                entries that made a record, latest record first, then the others by first arrival.  The device keeps lastRecord and
 *                firstArrival per entry; the front is the owner's largest lastRecord.  (tests/test_modrep1.py proves this against a replay.)
 *   verdicts     a lane per mod over its two lists; pre[0] comes from the persistent triple, which only a non-empty build overwrites.
 * Counts are added with integer atomics: sums and minima of integers do not depend on the order.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <vector>
#include <string>
#include <algorithm>
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_devsort.h"
#include "mg_modrep_int.h"

#define MG_REP1_MIN 5u                /* modrep.c:108,383,407 */

static thread_local U64 gRep1Diag[8];
extern "C" void mgRep1Diag (U64 out8[8]) { memcpy (out8, gRep1Diag, sizeof (gRep1Diag)); }

#define MG_FOR(i, n) for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < (n) ; i += (U64) gridDim.x * blockDim.x)

/* ---- n[], cleanMods ---- */

/* modrep.c:343: ++n[k] per hit; bad[0] |= 1 where k == max, 2 where k is beyond the set */
__global__ void mgRep1TallyKernel (const U32 *__restrict__ hitK, U64 n, U32 max, U32 *__restrict__ modN, U32 *__restrict__ bad)
{
  MG_FOR (h, n)
    { const U32 k = hitK[h];
      if (k >= max) atomicOr (bad, k == max ? 1u : 2u); else atomicAdd (&modN[k], 1u);
    }
}
/* hitRead[h] = the last read r < nReads with hitStart[r] <= h */
__global__ void mgRep1ReadOfHitKernel (const U32 *__restrict__ hitStart, U32 nReads, U64 n, U32 *__restrict__ hitRead)
{
  MG_FOR (h, n)
    { U32 lo = 0, hi = nReads - 1;
      while (lo < hi) { const U32 mid = lo + (hi - lo + 1) / 2; if ((U64) hitStart[mid] <= h) lo = mid; else hi = mid - 1; }
      hitRead[h] = lo;
    }
}
/* modrep.c:106-116 over i = 0 .. max - 1: tally[4] += mod0, small, big, good; the two middle classes are zeroed */
__global__ __launch_bounds__ (256)
void mgRep1CleanKernel (U32 *__restrict__ modN, U32 max, U32 thresh, U32 *__restrict__ tally)
{
  __shared__ U32 lds[4];
  U32 c[4] = { 0, 0, 0, 0 };
  MG_FOR (i, max)
    { const U32 n = modN[i];
      if (!n) ++c[0];
      else if (n < MG_REP1_MIN) { modN[i] = 0; ++c[1]; }
      else if (n > thresh) { modN[i] = 0; ++c[2]; }
      else ++c[3];
    }
  for (int j = 0 ; j < 4 ; ++j)
    { const U32 s = mgBlockReduce<256, MgSum> (c[j], lds);
      if (!threadIdx.x && s) atomicAdd (&tally[j], s);
    }
}
/* modrep.c:123: flag[h] = the hit's mod still counts, h < n; flag[n] = 0 */
__global__ void mgRep1LiveFlagKernel (const U32 *__restrict__ hitK, U64 n, const U32 *__restrict__ modN, U32 *__restrict__ flag)
{ MG_FOR (h, n + 1) flag[h] = h < n && modN[hitK[h]] != 0; }

/* ---- compaction ---- */

/* keepRead[r] for r < nReads, keepRead[nReads] = 0, from the reads' drop marks */
__global__ void mgRep1KeepReadKernel (const U32 *__restrict__ drop, U32 nReads, U32 *__restrict__ keepRead)
{ MG_FOR (r, (U64) nReads + 1) keepRead[r] = r < nReads && !drop[r]; }
__global__ void mgRep1KeepHitOfReadKernel (const U32 *__restrict__ hitRead, U64 n, const U32 *__restrict__ keepRead, U32 *__restrict__ flag)
{ MG_FOR (h, n + 1) flag[h] = h < n && keepRead[hitRead[h]] != 0; }
__global__ void mgRep1MoveReadsKernel (const U32 *__restrict__ keepRead, const U32 *__restrict__ readPlace, const U32 *__restrict__ readI, U32 nReads, U32 *__restrict__ readIOut)
{ MG_FOR (r, nReads) if (keepRead[r]) readIOut[readPlace[r]] = readI[r]; }
/* the kept hits to their places, in order; readPlace != 0: the reads are renumbered; count[r'] += 1 per kept hit */
__global__ void mgRep1MoveHitsKernel (const U32 *__restrict__ flag, const U32 *__restrict__ place, U64 n, const U32 *__restrict__ hitK, const U32 *__restrict__ hitX,
                                      const U32 *__restrict__ hitRead, const U32 *__restrict__ readPlace, U32 *__restrict__ outK, U32 *__restrict__ outX, U32 *__restrict__ outRead,
                                      U32 *__restrict__ count)
{
  MG_FOR (h, n)
    { if (!flag[h]) continue;
      const U32 p = place[h], r = readPlace ? readPlace[hitRead[h]] : hitRead[h];
      outK[p] = hitK[h]; outX[p] = hitX[h]; outRead[p] = r;
      atomicAdd (&count[r], 1u);
    }
}

/* ---- the run removal (modrep.c:356-369) ---- */

/* a wave per read.  Inside a read the kept hits are a chain: from xNext = 0, the first hit with x >= xNext is kept and sets xNext = x + K.
   The wave holds 64 positions in registers; a ballot finds the chain's next hit among them, a shuffle reads its x.  flag[h] = kept;
   a hit that is not kept takes 1 from its mod's n; removed[0] += their number */
__global__ __launch_bounds__ (256)
void mgRep1RunsKernel (const U32 *__restrict__ hitStart, U32 nReads, const U32 *__restrict__ hitK, const U32 *__restrict__ hitX, int K,
                       U32 *__restrict__ flag, U32 *__restrict__ modN, U32 *__restrict__ removed)
{
  const U32 lane = threadIdx.x & 63u, wavesPerBlock = blockDim.x >> 6;
  for (U64 r = (U64) blockIdx.x * wavesPerBlock + (threadIdx.x >> 6) ; r < nReads ; r += (U64) gridDim.x * wavesPerBlock)
    { const U32 s = hitStart[r], e = hitStart[r + 1];
      long long xNext = 0;
      U32 gone = 0;
      for (U32 base = s ; base < e ; base += 64)
        { const U32 h = base + lane;
          const bool valid = h < e;
          const int x = valid ? (int) hitX[h] : 0;
          bool keep = false;
          U32 from = 0;
          for (;;)
            { const U64 m = __ballot (valid && lane >= from && (long long) x >= xNext);
              if (!m) break;
              const U32 f = (U32) __ffsll ((long long) m) - 1u;
              xNext = (long long) __shfl (x, (int) f) + K;
              if (lane == f) keep = true;
              from = f + 1;
            }
          if (valid)
            { flag[h] = keep;
              if (!keep) { atomicSub (&modN[hitK[h]], 1u); ++gone; }
            }
        }
      gone = mgWaveReduce<MgSum> (gone);
      if (!lane && gone) atomicAdd (removed, gone);
    }
}
__global__ void mgRep1ZeroAtKernel (U32 *__restrict__ a, U64 at) { if (!blockIdx.x && !threadIdx.x) a[at] = 0; }

/* ---- buildPrePost (modrep.c:150-168) ---- */

/* flag[h] = hit h has a hit of its read before it, h < n; flag[n] = 0 */
__global__ void mgRep1LinkFlagKernel (const U32 *__restrict__ hitRead, const U32 *__restrict__ hitStart, U64 n, U32 *__restrict__ flag)
{ MG_FOR (h, n + 1) flag[h] = h < n && h > hitStart[hitRead[h]]; }
/* link t = place[h]: (k0, k1, dx, read); ++nPost[k0], ++nPre[k1] (modrep.c:164-165) */
__global__ void mgRep1LinkKernel (const U32 *__restrict__ flag, const U32 *__restrict__ place, U64 n, const U32 *__restrict__ hitK, const U32 *__restrict__ hitX, const U32 *__restrict__ hitRead,
                                  U32 *__restrict__ k0, U32 *__restrict__ k1, int *__restrict__ dx, U32 *__restrict__ lread, U32 *__restrict__ nPost, U32 *__restrict__ nPre)
{
  MG_FOR (h, n)
    { if (!flag[h]) continue;
      const U32 t = place[h], a = hitK[h - 1], b = hitK[h];
      k0[t] = a; k1[t] = b; dx[t] = (int) hitX[h] - (int) hitX[h - 1]; lread[t] = hitRead[h];
      atomicAdd (&nPost[a], 1u); atomicAdd (&nPre[b], 1u);
    }
}
__global__ void mgRep1GatherKernel (const U32 *__restrict__ key, const U32 *__restrict__ order, U64 n, U32 *__restrict__ out)
{ MG_FOR (i, n) out[i] = key[order[i]]; }
/* order[0 .. n): the links by (owner, partner), in arrival order inside a pair.  head[i] = position i starts a pair, head[n] = 0 */
__global__ void mgRep1HeadKernel (const U32 *__restrict__ order, U64 n, const U32 *__restrict__ owner, const U32 *__restrict__ partner, U32 *__restrict__ head)
{
  MG_FOR (i, n + 1)
    { U32 f = 0;
      if (i < n) { const U32 t = order[i]; f = 1; if (i) { const U32 q = order[i - 1]; f = owner[q] != owner[t] || partner[q] != partner[t]; } }
      head[i] = f;
    }
}
/* entry e = place[i] at a head: where it starts, whose it is, its first arrival; ++ownerEnt[owner].  entStart[nEnt] = n */
__global__ void mgRep1EntryKernel (const U32 *__restrict__ order, U64 n, const U32 *__restrict__ head, const U32 *__restrict__ place, const U32 *__restrict__ owner, const U32 *__restrict__ partner,
                                   U32 nEnt, U32 *__restrict__ entStart, U32 *__restrict__ entOwner, U32 *__restrict__ entPartner, U32 *__restrict__ entFirst, U32 *__restrict__ ownerEnt)
{
  MG_FOR (i, n + 1)
    { if (i == n) { entStart[nEnt] = (U32) n; continue; }
      if (!head[i]) continue;
      const U32 e = place[i], t = order[i];
      entStart[e] = (U32) i; entOwner[e] = owner[t]; entPartner[e] = partner[t]; entFirst[e] = t;
      atomicAdd (&ownerEnt[owner[t]], 1u);
    }
}
/* per link in sorted position i: its entry e, its occurrence number c = i - entStart[e] + 1; entX[e] += dx; the earliest arrival of the
   owner with this c: slot (ownerLink[owner] + c - 1) of first[], which lies inside the owner's own stretch of links, c being at most their number */
__global__ void mgRep1RankKernel (const U32 *__restrict__ order, U64 n, const U32 *__restrict__ head, const U32 *__restrict__ place, const U32 *__restrict__ entStart,
                                  const U32 *__restrict__ owner, const int *__restrict__ dx, const U32 *__restrict__ ownerLink,
                                  U32 *__restrict__ entOf, int *__restrict__ entX, U32 *__restrict__ first)
{
  MG_FOR (i, n)
    { const U32 e = place[i] + head[i] - 1u, t = order[i], c = (U32) i - entStart[e] + 1u;
      entOf[t] = e;
      atomicAdd (&entX[e], dx[t]);
      atomicMin (&first[ownerLink[owner[t]] + c - 1u], t);
    }
}
/* a link that is its owner's earliest with its c is a record: lastRecord[e] = max (ordinal + 1) */
__global__ void mgRep1RecordKernel (const U32 *__restrict__ order, U64 n, const U32 *__restrict__ entOf, const U32 *__restrict__ entStart, const U32 *__restrict__ owner,
                                    const U32 *__restrict__ ownerLink, const U32 *__restrict__ first, U32 *__restrict__ lastRecord)
{
  MG_FOR (i, n)
    { const U32 t = order[i], e = entOf[t], c = (U32) i - entStart[e] + 1u;
      if (first[ownerLink[owner[t]] + c - 1u] == t) atomicMax (&lastRecord[e], t + 1u);
    }
}
/* the front of a list: the entry with the owner's largest lastRecord */
__global__ void mgRep1FrontMaxKernel (const U32 *__restrict__ entOwner, const U32 *__restrict__ lastRecord, U32 nEnt, U32 *__restrict__ front)
{ MG_FOR (e, nEnt) atomicMax (&front[entOwner[e]], lastRecord[e]); }
/* pre[0] of every mod whose pre list is not empty now (modrep.c:376 reads it whether or not it is) */
__global__ void mgRep1FrontStoreKernel (const U32 *__restrict__ entOwner, const U32 *__restrict__ entPartner, const U32 *__restrict__ entStart, const int *__restrict__ entX,
                                        const U32 *__restrict__ lastRecord, U32 nEnt, const U32 *__restrict__ front, U32 *__restrict__ pre0K, U32 *__restrict__ pre0N, int *__restrict__ pre0X)
{
  MG_FOR (e, nEnt)
    { const U32 o = entOwner[e];
      if (lastRecord[e] != front[o]) continue;
      pre0K[o] = entPartner[e]; pre0N[o] = entStart[e + 1] - entStart[e]; pre0X[o] = entX[e];
    }
}

/* ---- the verdicts (modrep.c:374-391) ---- */

struct MgRep1Side { const U32 *ownerEntStart, *entPartner, *entStart; };      /* a side's lists: owner i's entries are [ownerEntStart[i], ownerEntStart[i + 1]) */

/* a lane per mod i < max with n[i]: zero[i] = 1 if it goes.  The tests read n[i] of the mod itself and nPre / nPost of others, which no
   verdict changes, so the mods are independent; n[] is zeroed here, in place.  stale[0] += mods with an empty pre list whose pre[0] holds an earlier build's entry */
__global__ void mgRep1VerdictKernel (U32 *__restrict__ modN, U32 max, const U32 *__restrict__ nPre, const U32 *__restrict__ nPost, MgRep1Side pre, MgRep1Side post,
                                     const U32 *__restrict__ pre0K, const U32 *__restrict__ pre0N, U32 *__restrict__ stale)
{
  MG_FOR (i, max)
    { const U32 n = modN[i];
      if (!n) continue;
      const U32 hn = pre0N[i], hk = pre0K[i];
      if (!nPre[i] && hn) atomicAdd (stale, 1u);
      if (hn == n && hn == nPost[hk]) { modN[i] = 0; continue; }      /* no new info in this mod */
      const U32 nThresh = n / 2;
      bool isBad = true;
      for (U32 e = pre.ownerEntStart[i] ; isBad && e < pre.ownerEntStart[i + 1] ; ++e)
        { const U32 c = pre.entStart[e + 1] - pre.entStart[e];
          if (c >= MG_REP1_MIN && (c > nThresh || c > nPost[pre.entPartner[e]] / 2)) isBad = false;
        }
      for (U32 e = post.ownerEntStart[i] ; isBad && e < post.ownerEntStart[i + 1] ; ++e)
        { const U32 c = post.entStart[e + 1] - post.entStart[e];
          if (c >= MG_REP1_MIN && (c > nThresh || c > nPre[post.entPartner[e]] / 2)) isBad = false;
        }
      if (isBad) modN[i] = 0;
    }
}

/* ---- weak links, n[] again ---- */

/* modrep.c:400-408: a link whose post entry has fewer than 5 occurrences marks its read */
__global__ void mgRep1WeakKernel (const U32 *__restrict__ entOf, const U32 *__restrict__ entStart, const U32 *__restrict__ lread, U64 nLinks, U32 *__restrict__ drop)
{ MG_FOR (t, nLinks) { const U32 e = entOf[t]; if (entStart[e + 1] - entStart[e] < MG_REP1_MIN) drop[lread[t]] = 1u; } }
/* modrep.c:419-423: j starts at 1 while h starts at hit 0: every hit of a read but its last */
__global__ void mgRep1RecountKernel (const U32 *__restrict__ hitK, const U32 *__restrict__ hitRead, const U32 *__restrict__ hitStart, U64 n, U32 *__restrict__ modN)
{ MG_FOR (h, n) if (h + 1 < hitStart[hitRead[h] + 1]) atomicAdd (&modN[hitK[h]], 1u); }

/* ---- -s2 ---- */

/* modrep.c:526-529: mask[read] |= bit j where the modimizer is the reference's entry boundary[j] */
__global__ void mgRep2MaskKernel (const U32 *__restrict__ ix, const U32 *__restrict__ rid, U64 n, U32 *__restrict__ mask)
{
  MG_FOR (i, n)
    { const U32 x = ix[i];
      const U32 b = x == 1u ? 1u : x == 961u ? 2u : x == 1951u ? 4u : x == 2961u ? 8u : 0u;      /* modrep.c:493-496 */
      if (b) atomicOr (&mask[rid[i]], b);
    }
}
/* modrep.c:531-534 */
__global__ __launch_bounds__ (256)
void mgRep2PairsKernel (const U32 *__restrict__ mask, U32 nReads, U32 *__restrict__ counts)
{
  __shared__ U32 lds[4];
  U32 c[4] = { 0, 0, 0, 0 };
  MG_FOR (r, nReads)
    { const U32 m = mask[r];
      for (int j = 0 ; j < 4 ; ++j) if ((m >> j & 1u) && (m >> ((j + 1) & 3) & 1u)) ++c[j];
    }
  for (int j = 0 ; j < 4 ; ++j)
    { const U32 s = mgBlockReduce<256, MgSum> (c[j], lds);
      if (!threadIdx.x && s) atomicAdd (&counts[j], s);
    }
}

/* ---------------------------------------------------------------------------------------- */

/* one side's lists of one build */
struct MgRep1Lists {
  U32 nEnt = 0;
  U32 *entStart = 0, *entOwner = 0, *entPartner = 0, *entFirst = 0, *lastRecord = 0, *entOf = 0, *ownerEntStart = 0;
  int *entX = 0;
  MgRep1Side side () const { MgRep1Side s = { ownerEntStart, entPartner, entStart }; return s; }
};

/* the state of a file's end on the device */
struct MgRep1End {
  MgDevScratch scratch;
  hipStream_t st = 0;
  U32 max = 0, nReads = 0; int K = 0;
  U64 N = 0, cap = 0;                                  /* hits now; the arrays' size */
  U32 readCap = 0;
  U32 *hitK = 0, *hitX = 0, *hitRead = 0, *altK = 0, *altX = 0, *altRead = 0;
  U32 *hitStart = 0, *count = 0, *readI = 0, *altReadI = 0, *drop = 0, *keepRead = 0, *readPlace = 0;
  U32 *flag = 0, *place = 0;
  U32 *modN = 0, *nPre = 0, *nPost = 0, *ownerLink = 0, *ownerEnt = 0, *front = 0, *pre0K = 0, *pre0N = 0; int *pre0X = 0;
  U32 *small = 0;                                      /* tally[4], removed, stale, bad */
  U32 *lk0 = 0, *lk1 = 0, *lread = 0, *key2 = 0, *first = 0; int *ldx = 0;
  U64 nLinks = 0;
  MgRep1Lists pre, post;
  U64 kernels = 0, builds = 0, maxLinks = 0, maxEntries = 0;
  MgRep1End () : scratch ("modrep -s1: the end of the file") {}
};
#define MG_R1_GO(S, kernel, n, ...) do { ++(S).kernels; hipLaunchKernelGGL (kernel, dim3 (mgGrid (n)), dim3 (256), 0, (S).st, __VA_ARGS__); } while (0)

static int mgRep1Alloc (MgRep1End &S)
{
  MgDevScratch &sc = S.scratch;
  const size_t c = (size_t) S.cap + 2, r = (size_t) S.readCap + 2, m = (size_t) S.max + 2;
  if (sc.get (&S.altK, c) || sc.get (&S.altX, c) || sc.get (&S.altRead, c) || sc.get (&S.flag, c) || sc.get (&S.place, c)
      || sc.get (&S.count, r) || sc.get (&S.altReadI, r) || sc.get (&S.drop, r) || sc.get (&S.keepRead, r) || sc.get (&S.readPlace, r)
      || sc.get (&S.modN, m) || sc.get (&S.nPre, m) || sc.get (&S.nPost, m) || sc.get (&S.ownerLink, m) || sc.get (&S.ownerEnt, m) || sc.get (&S.front, m)
      || sc.get (&S.pre0K, m) || sc.get (&S.pre0N, m) || sc.get (&S.pre0X, m) || sc.get (&S.small, 8)
      || sc.get (&S.lk0, c) || sc.get (&S.lk1, c) || sc.get (&S.lread, c) || sc.get (&S.key2, c) || sc.get (&S.first, c) || sc.get (&S.ldx, c)) return -1;
  for (MgRep1Lists *l : { &S.pre, &S.post })
    if (sc.get (&l->entStart, c) || sc.get (&l->entOwner, c) || sc.get (&l->entPartner, c) || sc.get (&l->entFirst, c) || sc.get (&l->lastRecord, c) || sc.get (&l->entOf, c)
        || sc.get (&l->entX, c) || sc.get (&l->ownerEntStart, m)) return -1;
  if (hipMemsetAsync (S.modN, 0, m * 4, S.st) != hipSuccess || hipMemsetAsync (S.pre0K, 0, m * 4, S.st) != hipSuccess || hipMemsetAsync (S.pre0N, 0, m * 4, S.st) != hipSuccess
      || hipMemsetAsync (S.pre0X, 0, m * 4, S.st) != hipSuccess || hipMemsetAsync (S.small, 0, 32, S.st) != hipSuccess) { sc.fail (); return -1; }      /* arrayCreate clears (array.c:63) */
  return 0;
}

/* the hits with flag[] set stay, in order; keepRead != 0 (with its scan in readPlace and newReads): the reads are renumbered, too */
static int mgRep1Compact (MgRep1End &S, bool byRead, U32 newReads)
{
  U32 newN = 0;
  if (mgExclusiveScan (S.scratch, S.flag, S.place, S.N + 1, S.st, &newN)) return -1;
  const U32 nr = byRead ? newReads : S.nReads;
  if (hipMemsetAsync (S.count, 0, ((size_t) nr + 1) * 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  if (byRead) MG_R1_GO (S, mgRep1MoveReadsKernel, S.nReads, S.keepRead, S.readPlace, S.readI, S.nReads, S.altReadI);
  MG_R1_GO (S, mgRep1MoveHitsKernel, S.N, S.flag, S.place, S.N, S.hitK, S.hitX, S.hitRead, byRead ? S.readPlace : (const U32 *) 0, S.altK, S.altX, S.altRead, S.count);
  if (hipGetLastError () != hipSuccess) { S.scratch.fail (); return -1; }
  if (mgExclusiveScan (S.scratch, S.count, S.hitStart, (U64) nr + 1, S.st)) return -1;
  std::swap (S.hitK, S.altK); std::swap (S.hitX, S.altX); std::swap (S.hitRead, S.altRead);
  if (byRead) std::swap (S.readI, S.altReadI);
  S.N = newN; S.nReads = nr;
  return 0;
}

/* cleanMods (modrep.c:97-127): the NMOD line, then the hits of the mods without a count leave */
static int mgRep1Clean (MgRep1End &S, FILE *out, int tally[4])
{
  U32 h[4];
  if (hipMemsetAsync (S.small, 0, 16, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  MG_R1_GO (S, mgRep1CleanKernel, S.max, S.modN, S.max, S.nReads / 2, S.small);
  MG_R1_GO (S, mgRep1LiveFlagKernel, S.N + 1, S.hitK, S.N, S.modN, S.flag);
  if (hipGetLastError () != hipSuccess || hipMemcpyAsync (h, S.small, 16, hipMemcpyDeviceToHost, S.st) != hipSuccess || hipStreamSynchronize (S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  for (int j = 0 ; j < 4 ; ++j) tally[j] = (int) h[j];
  if (out) fprintf (out, "NMOD mod0 %d modSmall %d modBig %d modGood %d\n", tally[0], tally[1], tally[2], tally[3]);      /* modrep.c:117 */
  return mgRep1Compact (S, false, 0);
}

/* one side of buildPrePost: the lists of every owner from the links */
static int mgRep1BuildSide (MgRep1End &S, MgRep1Lists &l, const U32 *owner, const U32 *partner, const U32 *ownerLinks, bool isPre)
{
  const size_t m = (size_t) S.max + 1;
  const U64 L = S.nLinks;
  l.nEnt = 0;
  if (hipMemsetAsync (S.ownerEnt, 0, (m + 1) * 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  if (L)
    { const int bits = mgKeyBits (S.max);
      U32 *byPartner = 0, *order = 0;
      if (mgRefStableSort (S.scratch, partner, 0, (U32) L, bits, &byPartner, S.st)) return -1;
      MG_R1_GO (S, mgRep1GatherKernel, L, owner, byPartner, L, S.key2);
      if (mgRefStableSort (S.scratch, S.key2, byPartner, (U32) L, bits, &order, S.st)) return -1;
      if (mgExclusiveScan (S.scratch, ownerLinks, S.ownerLink, m + 1, S.st)) return -1;      /* (ownerLinks[max + 1] is 0: the arrays have max + 2 entries) */
      MG_R1_GO (S, mgRep1HeadKernel, L + 1, order, L, owner, partner, S.flag);
      if (mgExclusiveScan (S.scratch, S.flag, S.place, L + 1, S.st, &l.nEnt)) return -1;
      if (hipMemsetAsync (l.entX, 0, (size_t) l.nEnt * 4, S.st) != hipSuccess || hipMemsetAsync (l.lastRecord, 0, (size_t) l.nEnt * 4, S.st) != hipSuccess
          || hipMemsetAsync (S.first, 0xff, L * 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
      MG_R1_GO (S, mgRep1EntryKernel, L + 1, order, L, S.flag, S.place, owner, partner, l.nEnt, l.entStart, l.entOwner, l.entPartner, l.entFirst, S.ownerEnt);
      MG_R1_GO (S, mgRep1RankKernel, L, order, L, S.flag, S.place, l.entStart, owner, S.ldx, S.ownerLink, l.entOf, l.entX, S.first);
      MG_R1_GO (S, mgRep1RecordKernel, L, order, L, l.entOf, l.entStart, owner, S.ownerLink, S.first, l.lastRecord);
      if (isPre)
        { if (hipMemsetAsync (S.front, 0, m * 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
          MG_R1_GO (S, mgRep1FrontMaxKernel, l.nEnt, l.entOwner, l.lastRecord, l.nEnt, S.front);
          MG_R1_GO (S, mgRep1FrontStoreKernel, l.nEnt, l.entOwner, l.entPartner, l.entStart, l.entX, l.lastRecord, l.nEnt, S.front, S.pre0K, S.pre0N, S.pre0X);
        }
      if (hipGetLastError () != hipSuccess) { S.scratch.fail (); return -1; }
    }
  return mgExclusiveScan (S.scratch, S.ownerEnt, l.ownerEntStart, m + 1, S.st) ? -1 : 0;
}

/* buildPrePost (modrep.c:150-168) */
static int mgRep1Build (MgRep1End &S)
{
  const size_t m = (size_t) S.max + 2;
  U32 L = 0;
  if (hipMemsetAsync (S.nPre, 0, m * 4, S.st) != hipSuccess || hipMemsetAsync (S.nPost, 0, m * 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  MG_R1_GO (S, mgRep1LinkFlagKernel, S.N + 1, S.hitRead, S.hitStart, S.N, S.flag);
  if (mgExclusiveScan (S.scratch, S.flag, S.place, S.N + 1, S.st, &L)) return -1;
  S.nLinks = L;
  MG_R1_GO (S, mgRep1LinkKernel, S.N, S.flag, S.place, S.N, S.hitK, S.hitX, S.hitRead, S.lk0, S.lk1, S.ldx, S.lread, S.nPost, S.nPre);
  if (hipGetLastError () != hipSuccess) { S.scratch.fail (); return -1; }
  if (mgRep1BuildSide (S, S.post, S.lk0, S.lk1, S.nPost, false) || mgRep1BuildSide (S, S.pre, S.lk1, S.lk0, S.nPre, true)) return -1;
  ++S.builds;
  if (L >= S.maxLinks) { S.maxLinks = L; S.maxEntries = S.post.nEnt; }
  return 0;
}

static int mgRep1Verdicts (MgRep1End &S)
{
  MG_R1_GO (S, mgRep1VerdictKernel, S.max, S.modN, S.max, S.nPre, S.nPost, S.pre.side (), S.post.side (), S.pre0K, S.pre0N, S.small + 5);
  if (hipGetLastError () != hipSuccess) { S.scratch.fail (); return -1; }
  return 0;
}

template <class T> static T *mgRep1Down (const void *d, size_t n)
{
  T *p = (T *) malloc ((n + 1) * sizeof (T));
  if (p && n && hipMemcpy (p, d, n * sizeof (T), hipMemcpyDeviceToHost) != hipSuccess) { free (p); p = 0; }
  return p;
}

/* a side's entries on the host, every owner's in list order: the entries that made a record, latest record first, then the others by
   first arrival (modrep.c:129-148; see the head of this file).  start[max + 2] */
static int mgRep1ListsToHost (const MgRep1End &S, const MgRep1Lists &l, U64 **start, int **k, int **n, int **x)
{
  const size_t m = (size_t) S.max + 1, ne = l.nEnt;
  U32 *es = mgRep1Down<U32> (l.entStart, ne + 1), *ep = mgRep1Down<U32> (l.entPartner, ne), *ef = mgRep1Down<U32> (l.entFirst, ne), *er = mgRep1Down<U32> (l.lastRecord, ne);
  U32 *os = mgRep1Down<U32> (l.ownerEntStart, m + 1);
  int *ex = mgRep1Down<int> (l.entX, ne);
  *start = (U64 *) malloc ((m + 1) * sizeof (U64)); *k = (int *) malloc ((ne + 1) * sizeof (int)); *n = (int *) malloc ((ne + 1) * sizeof (int)); *x = (int *) malloc ((ne + 1) * sizeof (int));
  int rc = (es && ep && ef && er && os && ex && *start && *k && *n && *x) ? 0 : -1;
  if (!rc)
    { std::vector<U32> ord;
      for (size_t i = 0 ; i <= m ; ++i) (*start)[i] = os[i];
      for (size_t i = 0 ; i < m ; ++i)
        { ord.clear ();
          for (U32 e = os[i] ; e < os[i + 1] ; ++e) ord.push_back (e);
          std::sort (ord.begin (), ord.end (), [&] (U32 a, U32 b)
            { if ((er[a] != 0) != (er[b] != 0)) return er[a] != 0;
              return er[a] ? er[a] > er[b] : ef[a] < ef[b]; });
          for (size_t j = 0 ; j < ord.size () ; ++j)
            { const U32 e = ord[j]; const size_t at = os[i] + j;
              (*k)[at] = (int) ep[e]; (*n)[at] = (int) (es[e + 1] - es[e]); (*x)[at] = ex[e];
            }
        }
    }
  free (es); free (ep); free (ef); free (er); free (os); free (ex);
  return rc;
}

extern "C" void mgRep1ResultFree (MgRep1Result *res)
{
  if (!res) return;
  free (res->modN); free (res->modNPre); free (res->modNPost); free (res->preStart); free (res->postStart);
  free (res->preK); free (res->preN); free (res->preX); free (res->postK); free (res->postN); free (res->postX);
  free (res->readI); free (res->hitStart); free (res->hitK);
  memset (res, 0, sizeof (*res));
}

/* the report (modrep.c:449-480) from what the last build left: the host formats, and sorts the reads */
static int mgRep1Report (MgRep1End &S, FILE *out, MgRep1Result *R)
{
  const size_t m = (size_t) S.max + 1;
  if (hipStreamSynchronize (S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  R->modN = mgRep1Down<int> (S.modN, m); R->modNPre = mgRep1Down<int> (S.nPre, m); R->modNPost = mgRep1Down<int> (S.nPost, m);
  int *readI = mgRep1Down<int> (S.readI, S.nReads), *hitK = mgRep1Down<int> (S.hitK, S.N);
  U32 *hs = mgRep1Down<U32> (S.hitStart, (size_t) S.nReads + 1);
  int rc = (R->modN && R->modNPre && R->modNPost && readI && hitK && hs) ? 0 : -1;
  if (!rc) rc = mgRep1ListsToHost (S, S.pre, &R->preStart, &R->preK, &R->preN, &R->preX) || mgRep1ListsToHost (S, S.post, &R->postStart, &R->postK, &R->postN, &R->postX) ? -1 : 0;
  R->readI = (int *) malloc (((size_t) S.nReads + 1) * sizeof (int)); R->hitStart = (U64 *) malloc (((size_t) S.nReads + 1) * sizeof (U64)); R->hitK = (int *) malloc ((S.N + 1) * sizeof (int));
  if (!R->readI || !R->hitStart || !R->hitK) rc = -1;
  if (!rc)
    { if (out)
        for (U32 i = 0 ; i < S.max ; ++i)                                                   /* modrep.c:450-461 */
          { if (!R->modN[i]) continue;
            fprintf (out, "MOD %d n %d pre %d (", (int) i, R->modN[i], R->modNPre[i]);
            for (U64 e = R->preStart[i] ; e < R->preStart[i + 1] ; ++e) fprintf (out, " %d:%d|%d:%d", R->preK[e], R->preN[e], R->modNPost[R->preK[e]], R->preX[e] / R->preN[e]);
            fprintf (out, ") post %d (", R->modNPost[i]);
            for (U64 e = R->postStart[i] ; e < R->postStart[i + 1] ; ++e) fprintf (out, " %d:%d|%d:%d", R->postK[e], R->postN[e], R->modNPre[R->postK[e]], R->postX[e] / R->postN[e]);
            fprintf (out, ")\n");
          }
      /* arraySort (reads, readOrder), modrep.c:79-90,463: lexicographic on the k sequences, the shorter first on a common prefix.  Equal
         reads stay in input order: glibc 2.35's qsort is a merge sort wherever it can allocate, and that is stable */
      std::vector<U32> ord (S.nReads);
      for (U32 r = 0 ; r < S.nReads ; ++r) ord[r] = r;
      auto cmp = [&] (U32 a, U32 b) { return std::lexicographical_compare (hitK + hs[a], hitK + hs[a + 1], hitK + hs[b], hitK + hs[b + 1]); };
      std::stable_sort (ord.begin (), ord.end (), cmp);
      U64 at = 0;
      int block = 0;
      for (U32 j = 0 ; j < S.nReads ; ++j)                                                   /* modrep.c:465-480: no BLOCK line after the last block */
        { const U32 r = ord[j];
          if (j && (cmp (ord[j - 1], r) || cmp (r, ord[j - 1])))
            { if (out)
                { fprintf (out, "BLOCK %3d", block);
                  for (U64 h = R->hitStart[j - 1] ; h < at ; ++h) fprintf (out, "\t%5d", R->hitK[h]);
                  fputc ('\n', out);
                }
              block = 0;
            }
          ++block;
          R->readI[j] = readI[r]; R->hitStart[j] = at;
          for (U32 h = hs[r] ; h < hs[r + 1] ; ++h) R->hitK[at++] = hitK[h];
          if (out)
            { fprintf (out, "READ %5d n %3d mods", readI[r], (int) (hs[r + 1] - hs[r]));
              for (U64 h = R->hitStart[j] ; h < at ; ++h) fprintf (out, "\t%5d", R->hitK[h]);
              fputc ('\n', out);
            }
        }
      R->hitStart[S.nReads] = at;
    }
  free (readI); free (hitK); free (hs);
  if (rc && !mgLastError ()[0]) mgSetError ("modrep -s1: the report could not be copied from the device");
  return rc;
}

/* modrep.c:354-480 on S: hitK / hitX / hitRead / hitStart / readI hold the file's hits, N and nReads their numbers */
static int mgRep1Run (MgRep1End &S, FILE *out, FILE *err, MgRep1Result *R, bool readLine)
{
  U32 bad = 0;
  MG_R1_GO (S, mgRep1TallyKernel, S.N, S.hitK, S.N, S.max, S.modN, S.small + 6);
  if (hipGetLastError () != hipSuccess || hipMemcpyAsync (&bad, S.small + 6, 4, hipMemcpyDeviceToHost, S.st) != hipSuccess || hipStreamSynchronize (S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  if (bad & 2u) { mgSetError ("modrep -s1: a hit lies beyond the second set's entries"); return -1; }
  if (bad) { mgSetError ("entry max of the second set occurs in a read, which modrep -s1 cannot represent (modrep.c:288,343: mods[] has max entries)"); return -1; }
  if (err && readLine) fprintf (err, "read %d reads, %d bad, %d good: \n", R->nRead, R->nBad, R->nGood);      /* modrep.c:351-352: the timing follows on that line */
  R->max = S.max;
  if (mgRep1Clean (S, out, R->nmod[0])) return -1;
  if (hipMemsetAsync (S.small + 4, 0, 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  ++S.kernels;
  hipLaunchKernelGGL (mgRep1RunsKernel, dim3 (mgGrid ((U64) S.nReads * 64)), dim3 (256), 0, S.st, S.hitStart, S.nReads, S.hitK, S.hitX, S.K, S.flag, S.modN, S.small + 4);
  MG_R1_GO (S, mgRep1ZeroAtKernel, 1, S.flag, S.N);
  if (hipGetLastError () != hipSuccess || mgRep1Compact (S, false, 0)) { if (!mgLastError ()[0]) S.scratch.fail (); return -1; }
  if (mgRep1Clean (S, out, R->nmod[1])) return -1;
  if (mgRep1Build (S) || mgRep1Verdicts (S) || mgRep1Clean (S, out, R->nmod[2])) return -1;      /* modrep.c:373-392 */
  if (mgRep1Build (S)) return -1;                                                                 /* modrep.c:395 */
  U32 kept = 0;
  if (hipMemsetAsync (S.drop, 0, ((size_t) S.nReads + 1) * 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  MG_R1_GO (S, mgRep1WeakKernel, S.nLinks, S.post.entOf, S.post.entStart, S.lread, S.nLinks, S.drop);
  MG_R1_GO (S, mgRep1KeepReadKernel, (U64) S.nReads + 1, S.drop, S.nReads, S.keepRead);
  if (hipGetLastError () != hipSuccess || mgExclusiveScan (S.scratch, S.keepRead, S.readPlace, (U64) S.nReads + 1, S.st, &kept)) { if (!mgLastError ()[0]) S.scratch.fail (); return -1; }
  MG_R1_GO (S, mgRep1KeepHitOfReadKernel, S.N + 1, S.hitRead, S.N, S.keepRead, S.flag);
  R->readsBefore = (int) S.nReads; R->readsAfter = (int) kept;
  if (mgRep1Compact (S, true, kept)) return -1;
  if (err) fprintf (err, "reduced %d reads to %d reads\n", R->readsBefore, R->readsAfter);      /* modrep.c:414 */
  if (hipMemsetAsync (S.modN, 0, ((size_t) S.max + 1) * 4, S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  MG_R1_GO (S, mgRep1RecountKernel, S.N, S.hitK, S.hitRead, S.hitStart, S.N, S.modN);
  if (mgRep1Clean (S, out, R->nmod[3])) return -1;
  if (mgRep1Build (S) || mgRep1Verdicts (S) || mgRep1Clean (S, out, R->nmod[4])) return -1;      /* modrep.c:427-446 */
  if (mgRep1Build (S)) return -1;                                                                 /* modrep.c:449 */
  U32 small[8];
  if (hipMemcpy (small, S.small, 32, hipMemcpyDeviceToHost) != hipSuccess) { S.scratch.fail (); return -1; }
  if (mgRep1Report (S, out, R)) return -1;
  const U64 d[8] = { S.builds, S.maxLinks, S.maxEntries, small[4], (U64) (R->readsBefore - R->readsAfter), small[5], S.kernels, 0 };
  memcpy (gRep1Diag, d, sizeof (d));
  return 0;
}

/* the arrays of the end for `cap` hits and `nReads` reads; hitStart and readI from the host */
static int mgRep1Begin (MgRep1End &S, U32 max, int K, U32 nReads, U64 N, const U32 *hHitStart, const int *hReadI)
{
  S.max = max; S.K = K; S.nReads = S.readCap = nReads; S.N = S.cap = N;
  if (mgRep1Alloc (S) || S.scratch.get (&S.hitStart, (size_t) nReads + 2) || S.scratch.get (&S.readI, (size_t) nReads + 2)) return -1;
  if (hipMemcpyAsync (S.hitStart, hHitStart, ((size_t) nReads + 1) * 4, hipMemcpyHostToDevice, S.st) != hipSuccess
      || (nReads && hipMemcpyAsync (S.readI, hReadI, (size_t) nReads * 4, hipMemcpyHostToDevice, S.st) != hipSuccess) || hipStreamSynchronize (S.st) != hipSuccess) { S.scratch.fail (); return -1; }
  return 0;
}

static int mgRep1Finish (int rc, MgRep1Result *R, MgRep1Result *res, const char *who)
{
  if (rc || !res) mgRep1ResultFree (R); else *res = *R;
  if (rc) { mgRepPathSet (-1); return mgFailedWith (who); }
  mgRepPathSet (0);
  return 0;
}

extern "C" int mgRepRunFinish1 (MgRepRun *run, FILE *out, FILE *err, MgRep1Result *res)
{
  mgRepPathSet (-1);
  memset (gRep1Diag, 0, sizeof (gRep1Diag));
  if (!run) { mgSetError ("mgRepRunFinish1: invalid arguments"); return -1; }
  MgRep1Result R; memset (&R, 0, sizeof (R));
  int rc = -1, cur = 0;
  if (mgEnsureDevice ()) rc = -1;
  else if (hipGetDevice (&cur) != hipSuccess || cur != run->device) mgSetError ("mgRepRunFinish1: the run was begun on GPU %d, the calling thread is on GPU %d", run->device, cur);
  else
    { MgRep1End S;
      const U32 nGood = (U32) run->goodI.size ();
      std::vector<U32> hs (run->hitStart.begin (), run->hitStart.end ());      /* (a file holds fewer than 2^32 - 16 hits: mgRepRunAdd) */
      R.nRead = (int) run->n.size (); R.nBad = run->nBad; R.nGood = (int) nGood;
      S.hitK = run->hitK.p; S.hitX = run->hitX.p; S.hitRead = run->hitRead.p;      /* (the run's own arrays are one of the two sets the compaction swaps between) */
      if (!run->nHit && (S.scratch.get (&S.hitK, 2) || S.scratch.get (&S.hitX, 2) || S.scratch.get (&S.hitRead, 2))) rc = -1;
      else rc = mgRep1Begin (S, run->ms->max, run->ms->hasher->k, nGood, run->nHit, hs.data (), run->goodI.data ()) || mgRep1Run (S, out, err, &R, true) ? -1 : 0;
    }
  delete run;
  return mgRep1Finish (rc, &R, res, "mgRepRunFinish1 failed");
}

extern "C" int mgRepAnalyze1File (MgRepRef *ref, const char *seqFile, const char *modFile, FILE *out, FILE *err, MgRep1Result *res)
{
  mgRepPathSet (-1);
  if (!ref || !seqFile || !modFile) { mgSetError ("mgRepAnalyze1File: invalid arguments"); return -1; }
  Modset *ms = mgRepReadSet (modFile);
  if (!ms) { if (!mgLastError ()[0]) mgSetError ("failed to read modset from file %s", modFile); return -1; }      /* modrep.c:284 */
  MgSeqReader *r = mgSeqOpen (seqFile);
  if (!r) { mgSetError ("can't open sequence file %s", seqFile); mgRepSetDestroy (ms); return -1; }      /* modrep.c:291 */
  MgRepRun *run = mgRepRunBegin (ref, ms);
  int rc = run ? 0 : -1;
  MgSeqBatch b;
  while (!rc && mgSeqNextBatch (r, MG_REP_FILE_BATCH, &b) > 0)
    { rc = mgRepRunAdd (run, b.bases, b.offsets, b.nSeq, 0);      /* modrep.c:305-310: a bad read prints nothing */
      mgSeqBatchFree (&b);
    }
  mgSeqClose (r);
  if (run)
    { if (rc) { const std::string msg = mgLastError (); mgRepRunFinish (run, 0, 0); mgSetError ("%s", msg.c_str ()); }
      else rc = mgRepRunFinish1 (run, out, err, res);
    }
  mgRepSetDestroy (ms);
  if (rc) mgRepPathSet (-1);
  return rc ? -1 : 0;
}

extern "C" int mgRepAnalyze1Hits (U32 max, int K, int nReads, const int *readI, const U64 *hitStart, const int *hitK, const int *hitX, FILE *out, FILE *err, MgRep1Result *res)
{
  mgRepPathSet (-1);
  memset (gRep1Diag, 0, sizeof (gRep1Diag));
  if (nReads < 0 || K < 0 || !hitStart || hitStart[0] != 0 || (nReads && !readI) || max >= 0xfffffff0u) { mgSetError ("mgRepAnalyze1Hits: invalid arguments"); return -1; }
  for (int r = 0 ; r < nReads ; ++r) if (hitStart[r + 1] < hitStart[r]) { mgSetError ("mgRepAnalyze1Hits: bad read starts"); return -1; }
  const U64 N = hitStart[nReads];
  if (N >= 0xfffffff0ull || (N && (!hitK || !hitX))) { mgSetError ("mgRepAnalyze1Hits: invalid arguments"); return -1; }
  for (U64 h = 0 ; h < N ; ++h)
    if (hitK[h] < 1 || (U32) hitK[h] > max || hitX[h] < 0 || hitX[h] > INT_MAX - K) { mgSetError ("mgRepAnalyze1Hits: hit %llu: 1 <= k <= max and 0 <= x <= INT_MAX - K", (unsigned long long) h); return -1; }
  if (mgEnsureDevice ()) return mgFailedWith ("mgRepAnalyze1Hits failed");
  MgRep1Result R; memset (&R, 0, sizeof (R));
  R.nGood = nReads;
  int rc;
  { MgRep1End S;
    std::vector<U32> hs (hitStart, hitStart + nReads + 1);
    rc = (S.scratch.get (&S.hitK, N + 2) || S.scratch.get (&S.hitX, N + 2) || S.scratch.get (&S.hitRead, N + 2) || mgRep1Begin (S, max, K, (U32) nReads, N, hs.data (), readI)) ? -1 : 0;
    if (!rc && N)
      { if (hipMemcpy (S.hitK, hitK, N * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy (S.hitX, hitX, N * 4, hipMemcpyHostToDevice) != hipSuccess) { S.scratch.fail (); rc = -1; }
        else { MG_R1_GO (S, mgRep1ReadOfHitKernel, N, S.hitStart, (U32) nReads, N, S.hitRead); if (hipGetLastError () != hipSuccess) { S.scratch.fail (); rc = -1; } }
      }
    if (!rc) rc = mgRep1Run (S, out, err, &R, false);
  }
  return mgRep1Finish (rc, &R, res, "mgRepAnalyze1Hits failed");
}

/* ---- -s2 ---- */

extern "C" int mgRepCount2 (MgRepRef *ref, const char *bases, const int64_t *offsets, int nReads, int counts4[4])
{
  mgRepPathSet (-1);
  if (!ref || !ref->ms || !ref->ms->hasher || !counts4 || nReads < 0 || (nReads && (!offsets || offsets[0] != 0 || (offsets[nReads] && !bases)))) { mgSetError ("mgRepCount2: invalid arguments"); return -1; }
  if (!nReads) { if (mgEnsureDevice ()) return -1; mgRepPathSet (0); return 0; }
  if ((U64) offsets[nReads] >= 0xffffff00ull) { mgSetError ("mgRepCount2: a batch holds fewer than 2^32 - 256 bases"); return -1; }
  for (int r = 0 ; r < nReads ; ++r)
    if (offsets[r + 1] < offsets[r] || offsets[r + 1] - offsets[r] > (int64_t) INT_MAX) { mgSetError ("mgRepCount2: bad read offsets"); return -1; }
  if (mgEnsureDevice ()) return -1;
  hipStream_t st = 0;
  MgDevScratch scratch ("modrep -s2 on the device");
  U32 *dPacked, *mask, *counts; U64 *dOff;
  MgRepSeeds a;
  U32 h[4];
  if (mgRepUpload (scratch, bases, offsets, (U32) nReads, (U64) offsets[nReads], &dPacked, &dOff, st)
      || mgRepSeedList (scratch, ref->ms, 0, dPacked, (U64) offsets[nReads], dOff, (U32) nReads, &a, st)) return mgFailedWith ("mgRepCount2 failed");
  if (scratch.get (&mask, (size_t) nReads) || scratch.get (&counts, 4)) return -1;
  if (hipMemsetAsync (mask, 0, (size_t) nReads * 4, st) != hipSuccess || hipMemsetAsync (counts, 0, 16, st) != hipSuccess) { scratch.fail (); return -1; }
  if (a.n) hipLaunchKernelGGL (mgRep2MaskKernel, dim3 (mgGrid (a.n)), dim3 (256), 0, st, a.ix, a.rid, a.n, mask);
  hipLaunchKernelGGL (mgRep2PairsKernel, dim3 (mgGrid ((U64) nReads, 256, 1024)), dim3 (256), 0, st, mask, (U32) nReads, counts);
  if (hipGetLastError () != hipSuccess || hipMemcpyAsync (h, counts, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess) { scratch.fail (); return -1; }
  for (int j = 0 ; j < 4 ; ++j) counts4[j] += (int) h[j];
  mgRepPathSet (0);
  return 0;
}

extern "C" int mgRepAnalyze2File (MgRepRef *ref, const char *seqFile, const char *modFile, FILE *out, int counts4[4])
{
  mgRepPathSet (-1);
  if (!ref || !seqFile || !modFile || !counts4) { mgSetError ("mgRepAnalyze2File: invalid arguments"); return -1; }
  Modset *ms = mgRepReadSet (modFile);                                            /* modrep.c:504-509: read, and not used */
  if (!ms) { if (!mgLastError ()[0]) mgSetError ("failed to read modset from file %s", modFile); return -1; }
  mgRepSetDestroy (ms);
  MgSeqReader *r = mgSeqOpen (seqFile);
  if (!r) { mgSetError ("can't open sequence file %s", seqFile); return -1; }      /* modrep.c:518 */
  for (int j = 0 ; j < 4 ; ++j) counts4[j] = 0;
  int rc = mgEnsureDevice () ? -1 : 0;
  MgSeqBatch b;
  while (!rc && mgSeqNextBatch (r, MG_REP_FILE_BATCH, &b) > 0)
    { rc = mgRepCount2 (ref, b.bases, b.offsets, b.nSeq, counts4);
      mgSeqBatchFree (&b);
    }
  mgSeqClose (r);
  if (rc) { mgRepPathSet (-1); return mgFailedWith ("mgRepAnalyze2File failed"); }
  if (out) fprintf (out, "n1 %d n2 %d n3 %d n4 %d\n", counts4[0], counts4[1], counts4[2], counts4[3]);      /* modrep.c:536 */
  mgRepPathSet (0);
  return 0;
}
