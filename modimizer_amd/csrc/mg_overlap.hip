/* mg_overlap.hip — the device side of modasm's overlap passes (-o1 / -o2 / -b / -c): the part of findOverlaps (modasm.c:314-418) that depends on
 * the hit lists and on info[] / depth[] alone, for a batch of query reads at once.  What depends on the order of the calls -- the reads' `bad` --
 * is replayed by the host (mg_rs_overlap.c), so the batches need no ordering between their kernels.
 *
 * Once per call (mgOvlDevOpen): hits, info[], the inverse lists, the reads' lengths; a hit's absolute position is the inclusive sum of its read's dx
 * (a wave per read).  Per batch (mgOvlDevBatch), every step a scan, a stable sort (mg_devsort.hip) or a kernel of independent threads:
 *   active hits   the batch's copy-1 hits sorted stably by (query, mod): the first of a run is the hit that hmap[] keeps (modasm.c:336-337), the others
 *                 are the query's repeats; the firsts, in that order, are the query's table (mod -> j + 1, with the orientation bit of x's hit)
 *   candidates    an active hit's candidates are its mod's inverse list, so the lists' lengths scanned IN HIT ORDER give every candidate its ordinal;
 *                 (query, y, ordinal) sorted stably by (query, y): a run's length is nHit, its first element's ordinal the arrival of y (modasm.c:340-345)
 *   pairs         the runs of 3 or more; a wave per pair walks y's hits against the query's table (mgOvPairKernel)
 *   order         a query's records by nHit descending, equal nHit by arrival: what a stable sort by nHit leaves (modasm.c:353)
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <vector>
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_xfer.h"
#include "mg_devsort.h"

#define MG_OV_LDS_DEFAULT 1024     /* table entries a wave stages in LDS: 8 KiB a wave, 32 KiB a workgroup of four -- five workgroups on a CU's 160 KiB, 20 of its 32 waves */
#define MG_OV_LDS_MAX     2048     /* 64 KiB a workgroup */
#define MG_OV_CAND_BYTES  48       /* device bytes a candidate takes at the peak (its two words, a sort's four arrays and histogram, the run marks) */

struct MgOvlDev {
  MgDevScratch scratch { "modasm's overlaps on the device" };
  U32 msMax = 0, nReads = 0; U64 totHit = 0;
  U8 *info = 0; U32 *hit = 0, *pos = 0, *invSpace = 0; U64 *hitStart = 0, *invStart = 0; int *len = 0;
  const U64 *hHitStart = 0;      /* the caller's, for the length of a batch */
};

static U32 mgOvGrid (U64 n) { const U64 g = (n + 255) / 256; return (U32) (g < 1 ? 1 : g > 65536 ? 65536 : g); }

/* pos[h] = the sum of dx over the hits of h's read up to and including h (xPos[j + 1], yPos at hit j: modasm.c:334,366,371); a wave per read */
__global__ __launch_bounds__ (256)
void mgOvPosKernel (const unsigned short *__restrict__ dx, const U64 *__restrict__ hitStart, U32 nReads, U32 *__restrict__ pos)
{
  const int lane = threadIdx.x & 63;
  for (U64 r = 1 + (U64) blockIdx.x * 4 + (threadIdx.x >> 6) ; r <= nReads ; r += (U64) gridDim.x * 4)
    { const U64 a = hitStart[r], e = hitStart[r + 1];
      U32 carry = 0;
      for (U64 b = a ; b < e ; b += 64)
        { const U64 i = b + lane;
          const U32 inc = mgWaveInclusiveSum (i < e ? (U32) dx[i] : 0u);
          if (i < e) pos[i] = carry + inc;
          carry += (U32) __shfl ((int) inc, 63);
        }
    }
}

/* the last q in 0 .. n - 1 with a[q] <= v (a ascending, a[0] <= v) */
__device__ __forceinline__ U32 mgOvLastLE (const U32 *__restrict__ a, U32 n, U32 v)
{
  U32 lo = 0, hi = n - 1;
  while (lo < hi) { const U32 mid = lo + (hi - lo + 1) / 2; if (a[mid] <= v) lo = mid; else hi = mid - 1; }
  return lo;
}

/* element e = hit j of query q (qStart[q] <= e < qStart[q + 1]): its query, and whether its mod is copy 1 */
__global__ __launch_bounds__ (256)
void mgOvElemKernel (U32 nElem, const U32 *__restrict__ qStart, U32 nq, const U32 *__restrict__ queries, const U64 *__restrict__ hitStart, const U32 *__restrict__ hit,
                     const U8 *__restrict__ info, U32 *__restrict__ eQ, U32 *__restrict__ flag)
{
  for (U64 e = (U64) blockIdx.x * blockDim.x + threadIdx.x ; e < nElem ; e += (U64) gridDim.x * blockDim.x)
    { const U32 q = mgOvLastLE (qStart, nq, (U32) e);
      const U32 m = hit[hitStart[queries[q]] + (e - qStart[q])] & MG_TOPMASK;
      eQ[e] = q; flag[e] = (info[m] & 3u) == 1u;
    }
}
/* the copy-1 elements in order: mod, element, query */
__global__ __launch_bounds__ (256)
void mgOvCompactKernel (U32 nElem, const U32 *__restrict__ flag, const U32 *__restrict__ place, const U32 *__restrict__ eQ, const U32 *__restrict__ qStart, const U32 *__restrict__ queries,
                        const U64 *__restrict__ hitStart, const U32 *__restrict__ hit, U32 *__restrict__ cMod, U32 *__restrict__ cElem, U32 *__restrict__ cQ)
{
  for (U64 e = (U64) blockIdx.x * blockDim.x + threadIdx.x ; e < nElem ; e += (U64) gridDim.x * blockDim.x)
    if (flag[e])
      { const U32 p = place[e], q = eQ[e];
        cMod[p] = hit[hitStart[queries[q]] + (e - qStart[q])] & MG_TOPMASK; cElem[p] = (U32) e; cQ[p] = q;
      }
}
__global__ __launch_bounds__ (256)
void mgOvGatherKernel (const U32 *__restrict__ idx, U32 n, const U32 *__restrict__ src, U32 xorWith, U32 *__restrict__ out)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x) out[i] = src[idx[i]] ^ xorWith; }

/* sorted[0 .. n1): the copy-1 elements by (query, mod), in hit order inside a run.  A run's first is active: it gets its mod's list as candidates and a
   line of the table; every other one is a repeat of its query */
__global__ __launch_bounds__ (256)
void mgOvActiveKernel (const U32 *__restrict__ sorted, U32 n1, const U32 *__restrict__ cMod, const U32 *__restrict__ cQ, const U64 *__restrict__ invStart,
                       U32 *__restrict__ tFlag, U32 *__restrict__ cnt, U32 *__restrict__ nRepeat)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n1 ; i += (U64) gridDim.x * blockDim.x)
    { const U32 p = sorted[i], m = cMod[p], q = cQ[p];
      bool first = true;
      if (i) { const U32 o = sorted[i - 1]; first = cMod[o] != m || cQ[o] != q; }
      tFlag[i] = first;
      cnt[p] = first ? (U32) (invStart[m + 1] - invStart[m]) : 0u;
      if (!first) atomicAdd (&nRepeat[q], 1u);
    }
}
/* the tables: per active hit, in (query, mod) order, its mod and (orientation bit of the query's hit) | (j + 1) */
__global__ __launch_bounds__ (256)
void mgOvTableKernel (const U32 *__restrict__ sorted, U32 n1, const U32 *__restrict__ tFlag, const U32 *__restrict__ tPlace, const U32 *__restrict__ cMod, const U32 *__restrict__ cElem,
                      const U32 *__restrict__ cQ, const U32 *__restrict__ qStart, const U32 *__restrict__ queries, const U64 *__restrict__ hitStart, const U32 *__restrict__ hit,
                      U32 *__restrict__ tabMod, U32 *__restrict__ tabVal, U32 *__restrict__ tabQ)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n1 ; i += (U64) gridDim.x * blockDim.x)
    if (tFlag[i])
      { const U32 t = tPlace[i], p = sorted[i], q = cQ[p], j = cElem[p] - qStart[q];
        tabMod[t] = cMod[p]; tabQ[t] = q;
        tabVal[t] = (hit[hitStart[queries[q]] + j] & MG_TOPBIT) | (j + 1);
      }
}
/* start[q] = the first place of keyQ[0 .. n) (ascending) that holds q or more, for q = 0 .. nq */
__global__ __launch_bounds__ (256)
void mgOvStartKernel (const U32 *__restrict__ keyQ, U32 n, U32 nq, U32 *__restrict__ start)
{
  for (U64 q = (U64) blockIdx.x * blockDim.x + threadIdx.x ; q <= nq ; q += (U64) gridDim.x * blockDim.x)
    { U32 lo = 0, hi = n;
      while (lo < hi) { const U32 mid = lo + (hi - lo) / 2; if (keyQ[mid] < q) lo = mid + 1; else hi = mid; }
      start[q] = lo;
    }
}
/* candidate c: entry c - cOff[p] of the list of the active element p with cOff[p] <= c < cOff[p] + cnt[p] (the last p with cOff[p] <= c: an element
   without candidates shares its offset with the next one, which comes later) */
__global__ __launch_bounds__ (256)
void mgOvEmitKernel (U32 nCand, const U32 *__restrict__ cOff, U32 n1, const U32 *__restrict__ cMod, const U32 *__restrict__ cQ, const U64 *__restrict__ invStart,
                     const U32 *__restrict__ invSpace, U32 *__restrict__ candY, U32 *__restrict__ candQ)
{
  for (U64 c = (U64) blockIdx.x * blockDim.x + threadIdx.x ; c < nCand ; c += (U64) gridDim.x * blockDim.x)
    { const U32 p = mgOvLastLE (cOff, n1, (U32) c);
      candY[c] = invSpace[invStart[cMod[p]] + ((U32) c - cOff[p])]; candQ[c] = cQ[p];
    }
}
/* sorted[0 .. n): the candidates by (query, y), in ordinal order inside a run */
__global__ __launch_bounds__ (256)
void mgOvHeadKernel (const U32 *__restrict__ sorted, U32 n, const U32 *__restrict__ candY, const U32 *__restrict__ candQ, U32 *__restrict__ head)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { bool h = true;
      if (i) { const U32 a = sorted[i - 1], b = sorted[i]; h = candY[a] != candY[b] || candQ[a] != candQ[b]; }
      head[i] = h;
    }
}
__global__ __launch_bounds__ (256)
void mgOvRunStartKernel (const U32 *__restrict__ head, const U32 *__restrict__ rid, U32 n, U32 nRuns, U32 *__restrict__ runStart)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { if (head[i]) runStart[rid[i]] = (U32) i;
      if (!i) runStart[nRuns] = n;
    }
}
__global__ __launch_bounds__ (256)
void mgOvKeepKernel (const U32 *__restrict__ runStart, U32 nRuns, U32 *__restrict__ keep)
{ for (U64 r = (U64) blockIdx.x * blockDim.x + threadIdx.x ; r < nRuns ; r += (U64) gridDim.x * blockDim.x) keep[r] = runStart[r + 1] - runStart[r] >= 3u; }
__global__ __launch_bounds__ (256)
void mgOvPairInitKernel (const U32 *__restrict__ runStart, U32 nRuns, const U32 *__restrict__ keep, const U32 *__restrict__ kPlace, const U32 *__restrict__ sorted,
                         const U32 *__restrict__ candY, const U32 *__restrict__ candQ, U32 *__restrict__ pairQ, U32 *__restrict__ pairY, U32 *__restrict__ pairN, U32 *__restrict__ pairFirst)
{
  for (U64 r = (U64) blockIdx.x * blockDim.x + threadIdx.x ; r < nRuns ; r += (U64) gridDim.x * blockDim.x)
    if (keep[r])
      { const U32 k = kPlace[r], c = sorted[runStart[r]];
        pairQ[k] = candQ[c]; pairY[k] = candY[c]; pairN[k] = runStart[r + 1] - runStart[r]; pairFirst[k] = c;
      }
}

/* One wave per pair (x = queries[pairQ], y = pairY): modasm.c:359-390 in one walk of y's hits, 64 at a time.  A lane looks its hit's mod up in the
   query's table by binary search -- the table staged in LDS if it has at most ldsCap entries, else in HBM.  The two order tests (ihx below the previous
   match's for the plus branch, above it for the minus branch; before the first match the previous is 0, resp. x's nHit) depend on the sequence of
   matches alone, so both are counted and the majority picks one at the end.  "The previous match" of a lane is the nearest matching lane below it in the
   stride (ballot, then a shuffle from that lane), or the last match of the strides before, which the wave carries along with the places of the first
   and the last match (isContained: modasm.c:373-377). */
__global__ __launch_bounds__ (256)
void mgOvPairKernel (U32 nPairs, const U32 *__restrict__ pairQ, const U32 *__restrict__ pairY, const U32 *__restrict__ pairN, const U32 *__restrict__ queries,
                     const U32 *__restrict__ tabStart, const U32 *__restrict__ tabMod, const U32 *__restrict__ tabVal, const U32 *__restrict__ hit, const U32 *__restrict__ pos,
                     const U64 *__restrict__ hitStart, const int *__restrict__ len, U32 ldsCap, MgOvlRec *__restrict__ rec)
{
  extern __shared__ U32 sTab[];                                       /* four waves x (ldsCap mods, ldsCap values) */
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const U64 k = (U64) blockIdx.x * 4 + w;
  const bool live = k < nPairs;
  U32 x = 0, y = 0, nT = 0;
  const U32 *tm = tabMod, *tv = tabVal;
  if (live) { const U32 q = pairQ[k]; y = pairY[k]; x = queries[q]; const U32 t0 = tabStart[q]; nT = tabStart[q + 1] - t0; tm += t0; tv += t0; }
  const bool inLds = nT <= ldsCap;
  U32 *lm = sTab + (size_t) w * 2 * ldsCap, *lv = lm + ldsCap;
  if (live && inLds) for (U32 i = lane ; i < nT ; i += 64) { lm[i] = tm[i]; lv[i] = tv[i]; }
  __syncthreads ();
  if (!live) return;
  const U64 xa = hitStart[x], ya = hitStart[y];
  const U32 xN = (U32) (hitStart[x + 1] - xa), yN = (U32) (hitStart[y + 1] - ya);
  U32 cPlus = 0, cMinus = 0, cLess = 0, cGreater = 0;                /* a lane's share */
  bool any = false; U32 prev = 0, firstJ = 0, firstIhx = 0, lastJ = 0;      /* the wave's: the same in every lane */
  for (U32 base = 0 ; base < yN ; base += 64)
    { const U32 j = base + lane;
      U32 hy = 0, val = 0;
      if (j < yN)
        { hy = hit[ya + j];
          const U32 m = hy & MG_TOPMASK;
          U32 lo = 0, hi = nT;
          while (lo < hi) { const U32 mid = lo + (hi - lo) / 2; if ((inLds ? lm[mid] : tm[mid]) < m) lo = mid + 1; else hi = mid; }
          if (lo < nT && (inLds ? lm[lo] : tm[lo]) == m) val = inLds ? lv[lo] : tv[lo];
        }
      const bool match = val != 0;                                   /* (j + 1 >= 1) */
      const U32 ihx = val & MG_TOPMASK;
      const U64 bal = __ballot (match);
      if (!bal) continue;
      const U64 below = bal & (((U64) 1 << lane) - 1);
      const U32 fromLane = (U32) __shfl ((int) ihx, below ? 63 - __clzll ((long long) below) : lane);
      if (match)
        { if (((hy ^ val) & MG_TOPBIT) == 0) ++cPlus; else ++cMinus;
          const bool has = below != 0 || any;
          const U32 before = below ? fromLane : prev;
          if (ihx < (has ? before : 0u)) ++cLess;
          if (ihx > (has ? before : xN)) ++cGreater;
        }
      const int top = 63 - __clzll ((long long) bal), bottom = __ffsll ((unsigned long long) bal) - 1;
      const U32 ihxBottom = (U32) __shfl ((int) ihx, bottom);
      prev = (U32) __shfl ((int) ihx, top); lastJ = base + (U32) top;
      if (!any) { any = true; firstJ = base + (U32) bottom; firstIhx = ihxBottom; }
    }
  U32 nPlus = mgWaveReduce<MgSum> (cPlus), nMinus = mgWaveReduce<MgSum> (cMinus);
  const U32 nLess = mgWaveReduce<MgSum> (cLess), nGreater = mgWaveReduce<MgSum> (cGreater);
  if (lane) return;
  MgOvlRec r; r.iy = y; r.nHit = (U16) pairN[k]; r.nBadOrder = r.nBadFlip = r.flags = 0;
  if (nPlus > nMinus)
    { r.flags = 1; r.nBadFlip = (U16) nMinus; r.nBadOrder = (U16) nLess; nPlus -= nLess;
      if (any)
        { const long long firstDiff = (long long) pos[xa + firstIhx - 1] - (long long) pos[ya + firstJ];
          const long long lastDiff = (long long) pos[xa + prev - 1] - (long long) pos[ya + lastJ];
          if (firstDiff < 0 && !((long long) len[x] - lastDiff > (long long) len[y])) r.flags |= 2;
        }
    }
  else if (nMinus && !nPlus) { r.nBadOrder = (U16) nGreater; nMinus -= nGreater; }
  r.nPlus = (U16) nPlus; r.nMinus = (U16) nMinus;
  rec[k] = r;
}
__global__ __launch_bounds__ (256)
void mgOvOutKernel (const U32 *__restrict__ order, U32 n, const MgOvlRec *__restrict__ rec, const U32 *__restrict__ pairQ, MgOvlRec *__restrict__ outRec, U32 *__restrict__ outQ)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x) { const U32 o = order[i]; outRec[i] = rec[o]; outQ[i] = pairQ[o]; } }

/* ---------------------------------------------------------------------------------------- */

extern "C" U64 mgOvlDevCandBudget (void)
{
  size_t freeB = 0;
  if (!mgDevFreeBytes (&freeB)) return (U64) 1 << 20;
  U64 b = (U64) freeB / 3 / MG_OV_CAND_BYTES;
  if (b < ((U64) 1 << 16)) b = (U64) 1 << 16;
  if (b > ((U64) 1 << 30)) b = (U64) 1 << 30;
  return b;
}

extern "C" void mgOvlDevClose (MgOvlDev *d) { delete d; }

extern "C" int mgOvlDevOpen (MgOvlDev **out, const MgRsView *v)
{
  *out = 0;
  if (mgEnsureDevice ()) return -1;
  const U32 msMax = v->msMax, nReads = v->nReads; const U64 totHit = v->totHit;
  const size_t m = (size_t) msMax + 1;
  const U64 listed = v->invStart[m];
  size_t freeB = 0;
  const size_t need = m + m * 8 + 16 + (totHit + 1) * 10 + (listed + 1) * 4 + ((size_t) nReads + 3) * 12 + ((size_t) 128 << 20);      /* and room for a batch */
  if (!mgDevFreeBytes (&freeB) || need >= freeB) return 1;
  MgOvlDev *d = new MgOvlDev;
  d->msMax = msMax; d->nReads = nReads; d->totHit = totHit; d->hHitStart = v->hitStart;
  MgDevScratch tmp ("modasm's overlaps on the device");
  unsigned short *dDx;
  if (d->scratch.get (&d->info, m) || d->scratch.get (&d->invStart, m + 1) || d->scratch.get (&d->hit, totHit + 1) || d->scratch.get (&d->pos, totHit + 1)
      || d->scratch.get (&d->invSpace, listed + 1) || d->scratch.get (&d->hitStart, (size_t) nReads + 3) || d->scratch.get (&d->len, (size_t) nReads + 2) || tmp.get (&dDx, totHit + 1)
      || hipDeviceSynchronize ())
    { delete d; return -1; }
  if (mgXferH2D (d->info, v->info, m) || mgXferH2D (d->invStart, v->invStart, (m + 1) * 8) || mgXferH2D (d->hitStart, v->hitStart, ((size_t) nReads + 2) * 8)
      || mgXferH2D (d->len, v->len, ((size_t) nReads + 1) * sizeof (int))
      || (totHit && (mgXferH2D (d->hit, v->hit, totHit * 4) || mgXferH2D (dDx, v->dx, totHit * 2))) || (listed && mgXferH2D (d->invSpace, v->invSpace, listed * 4)))
    { delete d; return -1; }
  if (nReads && totHit) MG_LAUNCH (MG_K_OVL_ACTIVE, 0, mgOvPosKernel, dim3 (mgOvGrid ((U64) nReads * 64)), dim3 (256), 0, 0, dDx, d->hitStart, nReads, d->pos);
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (0) != hipSuccess) { tmp.fail (); delete d; return -1; }
  *out = d;
  return 0;
}

/* values (or the positions) by keys, stable, timed as one of the overlap sorts */
static MgStatus mgOvSort (MgDevScratch &scratch, const U32 *keys, const U32 *vals, U32 n, U64 maxKey, U32 **out, hipStream_t st)
{
  mgProfBegin (MG_K_OVL_SORT, st);
  const MgStatus s = mgRefStableSort (scratch, keys, vals, n, mgKeyBits (maxKey), out, st);
  mgProfEnd (MG_K_OVL_SORT, st);
  return s;
}
#define OV_LAUNCH(id, kernel, n, ...) MG_LAUNCH (id, st, kernel, dim3 (mgOvGrid (n)), dim3 (256), 0, st, __VA_ARGS__)

extern "C" int mgOvlDevBatch (MgOvlDev *d, const U32 *queries, U32 nq, U32 *nRepeat, U64 *start, MgOvlRec **recsOut, U64 diag[4])
{
  *recsOut = 0;
  hipStream_t st = 0;
  const MgKnobs *kn = mgKnobs ();
  const U32 ldsCap = kn->overlapLds == MG_KNOB_UNSET || kn->overlapLds < 0 ? MG_OV_LDS_DEFAULT : kn->overlapLds > MG_OV_LDS_MAX ? MG_OV_LDS_MAX : (U32) kn->overlapLds;
  /* the batch's elements: the hits of its queries, query after query (fewer than 2^31: the caller's batches) */
  std::vector<U32> hQStart ((size_t) nq + 1);
  U64 nElem64 = 0;
  for (U32 q = 0 ; q < nq ; ++q) { hQStart[q] = (U32) nElem64; nElem64 += d->hHitStart[queries[q] + 1] - d->hHitStart[queries[q]]; }
  hQStart[nq] = (U32) nElem64;
  if (nElem64 >= 0x7fffffffull) { mgSetError ("overlaps: a batch of 2^31 hits or more"); return -1; }
  const U32 nElem = (U32) nElem64;
  for (U32 q = 0 ; q < nq ; ++q) nRepeat[q] = 0;
  for (U32 q = 0 ; q <= nq ; ++q) start[q] = 0;
  MgOvlRec *recs = (MgOvlRec *) malloc (sizeof (MgOvlRec));
  if (!recs) { mgSetError ("overlaps: out of memory"); return -1; }
  *recsOut = recs;
  if (!nElem) return 0;
  size_t freeB = 0;
  if (!mgDevFreeBytes (&freeB) || (size_t) nElem * 44 + ((size_t) 64 << 20) >= freeB) { free (recs); *recsOut = 0; return 1; }
  MgDevScratch scratch ("modasm's overlaps on the device");
  U32 *dQStart, *dQueries, *dRepeat, *eQ, *flag, *place;
  if (scratch.get (&dQStart, (size_t) nq + 1) || scratch.get (&dQueries, nq) || scratch.get (&dRepeat, nq) || scratch.get (&eQ, nElem) || scratch.get (&flag, nElem) || scratch.get (&place, nElem)) goto failed;
  if (hipMemcpyAsync (dQStart, hQStart.data (), ((size_t) nq + 1) * 4, hipMemcpyHostToDevice, st) || hipMemcpyAsync (dQueries, queries, (size_t) nq * 4, hipMemcpyHostToDevice, st)
      || hipMemsetAsync (dRepeat, 0, (size_t) nq * 4, st)) { scratch.fail (); goto failed; }
  {
    /* ---- active hits, the tables, the candidates' places ---- */
    U32 n1 = 0, nTab = 0, nCand = 0, nRuns = 0, nPairs = 0;
    OV_LAUNCH (MG_K_OVL_ACTIVE, mgOvElemKernel, nElem, nElem, dQStart, nq, dQueries, d->hitStart, d->hit, d->info, eQ, flag);
    if (mgExclusiveScan (scratch, flag, place, nElem, st, &n1)) goto failed;
    if (!n1) return 0;                                                /* no copy-1 hit: no repeats, no partners */
    U32 *cMod, *cElem, *cQ, *byMod, *keyQ, *byQMod, *tFlag, *tPlace, *cnt, *cOff, *tabMod, *tabVal, *tabQ, *tabStart;
    if (scratch.get (&cMod, n1) || scratch.get (&cElem, n1) || scratch.get (&cQ, n1) || scratch.get (&keyQ, n1) || scratch.get (&tFlag, n1) || scratch.get (&tPlace, n1)
        || scratch.get (&cnt, n1) || scratch.get (&cOff, n1) || scratch.get (&tabStart, (size_t) nq + 1)) goto failed;
    OV_LAUNCH (MG_K_OVL_ACTIVE, mgOvCompactKernel, nElem, nElem, flag, place, eQ, dQStart, dQueries, d->hitStart, d->hit, cMod, cElem, cQ);
    if (mgOvSort (scratch, cMod, 0, n1, d->msMax, &byMod, st)) goto failed;
    OV_LAUNCH (MG_K_OVL_ACTIVE, mgOvGatherKernel, n1, byMod, n1, cQ, 0u, keyQ);
    if (mgOvSort (scratch, keyQ, byMod, n1, nq, &byQMod, st)) goto failed;
    OV_LAUNCH (MG_K_OVL_ACTIVE, mgOvActiveKernel, n1, byQMod, n1, cMod, cQ, d->invStart, tFlag, cnt, dRepeat);
    if (mgExclusiveScan (scratch, tFlag, tPlace, n1, st, &nTab) || mgExclusiveScan (scratch, cnt, cOff, n1, st, &nCand)) goto failed;
    if (scratch.get (&tabMod, (size_t) nTab + 1) || scratch.get (&tabVal, (size_t) nTab + 1) || scratch.get (&tabQ, (size_t) nTab + 1)) goto failed;
    OV_LAUNCH (MG_K_OVL_ACTIVE, mgOvTableKernel, n1, byQMod, n1, tFlag, tPlace, cMod, cElem, cQ, dQStart, dQueries, d->hitStart, d->hit, tabMod, tabVal, tabQ);
    OV_LAUNCH (MG_K_OVL_ACTIVE, mgOvStartKernel, (U64) nq + 1, tabQ, nTab, nq, tabStart);
    if (hipMemcpyAsync (nRepeat, dRepeat, (size_t) nq * 4, hipMemcpyDeviceToHost, st) || hipStreamSynchronize (st)) { scratch.fail (); goto failed; }
    diag[1] += nCand;
    if (nCand >= 0x7fffffffu) { mgSetError ("overlaps: a batch of 2^31 candidates or more"); goto failed; }
    if (!nCand) return 0;
    if (!mgDevFreeBytes (&freeB) || (size_t) nCand * MG_OV_CAND_BYTES + ((size_t) 64 << 20) >= freeB) { free (recs); *recsOut = 0; return 1; }
    /* ---- the candidates, grouped by (query, y) ---- */
    U32 *candY, *candQ, *byY, *keyCQ, *byQY, *head, *rid, *runStart, *keep, *kPlace;
    if (scratch.get (&candY, nCand) || scratch.get (&candQ, nCand) || scratch.get (&keyCQ, nCand) || scratch.get (&head, nCand) || scratch.get (&rid, nCand)) goto failed;
    OV_LAUNCH (MG_K_OVL_EMIT, mgOvEmitKernel, nCand, nCand, cOff, n1, cMod, cQ, d->invStart, d->invSpace, candY, candQ);
    if (mgOvSort (scratch, candY, 0, nCand, d->nReads, &byY, st)) goto failed;
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvGatherKernel, nCand, byY, nCand, candQ, 0u, keyCQ);
    if (mgOvSort (scratch, keyCQ, byY, nCand, nq, &byQY, st)) goto failed;
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvHeadKernel, nCand, byQY, nCand, candY, candQ, head);
    if (mgExclusiveScan (scratch, head, rid, nCand, st, &nRuns)) goto failed;
    if (scratch.get (&runStart, (size_t) nRuns + 1) || scratch.get (&keep, nRuns) || scratch.get (&kPlace, nRuns)) goto failed;
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvRunStartKernel, nCand, head, rid, nCand, nRuns, runStart);
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvKeepKernel, nRuns, runStart, nRuns, keep);
    if (mgExclusiveScan (scratch, keep, kPlace, nRuns, st, &nPairs)) goto failed;
    diag[2] += nPairs;
    if (!nPairs) return 0;
    /* ---- the pairs ---- */
    U32 *pairQ, *pairY, *pairN, *pairFirst, *byFirst, *keyN, *byN, *keyPQ, *order, *outQ, *dStart; MgOvlRec *rec, *outRec;
    if (scratch.get (&pairQ, nPairs) || scratch.get (&pairY, nPairs) || scratch.get (&pairN, nPairs) || scratch.get (&pairFirst, nPairs) || scratch.get (&keyN, nPairs)
        || scratch.get (&keyPQ, nPairs) || scratch.get (&outQ, nPairs) || scratch.get (&dStart, (size_t) nq + 1) || scratch.get (&rec, nPairs) || scratch.get (&outRec, nPairs)) goto failed;
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvPairInitKernel, nRuns, runStart, nRuns, keep, kPlace, byQY, candY, candQ, pairQ, pairY, pairN, pairFirst);
    MG_LAUNCH (MG_K_OVL_PAIR, st, mgOvPairKernel, dim3 ((nPairs + 3) / 4), dim3 (256), (size_t) ldsCap * 32, st, nPairs, pairQ, pairY, pairN, dQueries, tabStart, tabMod, tabVal,
               d->hit, d->pos, d->hitStart, d->len, ldsCap, rec);
    ++diag[3];
    /* a query's records by nHit descending, equal nHit by arrival: by arrival, then stably by 65535 - nHit, then stably by query */
    if (mgOvSort (scratch, pairFirst, 0, nPairs, nCand, &byFirst, st)) goto failed;
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvGatherKernel, nPairs, byFirst, nPairs, pairN, 0xffffu, keyN);      /* (nHit < 65535: the lists it counts are shorter) */
    if (mgOvSort (scratch, keyN, byFirst, nPairs, 0xffffu, &byN, st)) goto failed;
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvGatherKernel, nPairs, byN, nPairs, pairQ, 0u, keyPQ);
    if (mgOvSort (scratch, keyPQ, byN, nPairs, nq, &order, st)) goto failed;
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvOutKernel, nPairs, order, nPairs, rec, pairQ, outRec, outQ);
    OV_LAUNCH (MG_K_OVL_RUNS, mgOvStartKernel, (U64) nq + 1, outQ, nPairs, nq, dStart);
    std::vector<U32> hStart ((size_t) nq + 1);
    if (hipGetLastError () != hipSuccess || hipMemcpyAsync (hStart.data (), dStart, ((size_t) nq + 1) * 4, hipMemcpyDeviceToHost, st) || hipStreamSynchronize (st)) { scratch.fail (); goto failed; }
    free (recs);
    *recsOut = recs = (MgOvlRec *) malloc ((size_t) nPairs * sizeof (MgOvlRec));
    if (!recs) { mgSetError ("overlaps: out of memory"); goto failed; }
    if (mgXferD2H (recs, outRec, (size_t) nPairs * sizeof (MgOvlRec), MG_XFER_COPY)) goto failed;
    for (U32 q = 0 ; q <= nq ; ++q) start[q] = hStart[q];
    return 0;
  }
failed:
  free (*recsOut); *recsOut = 0;
  return -1;
}
