/* mg_rdna.hip — the device side of modasm -R and -T (refFlag, modasm.c:752-860; testMods, 595-748) for a read set that is on the host.
 *
 * -R: per read the hit number of the 200th hit on a core-and-reference mod from either end (modasm.c:781-802), a wave per read: ballots of
 * 64 hits, their popcounts added up, the lane of the 200th picked by its rank in the ballot.  The walk between the two numbers depends on the
 * order of the reads and is the host's (mg_rs_rdna.c).
 *
 * -T: the reference gathers, per tested mod i and per read that holds it, one (partner mod, signed distance) for every other hit that passes
 * checkMod, sorts them, and then uses per partner m only the count and the first and the last distance.  Count, min and max are commutative
 * integer reductions: no sort, and any order of accumulation gives the same bits.  Tested mods are taken in batches; per batch
 *   mgRdnaVisitKernel    a wave per visit (entry of inv[i]): the FIRST occurrence of i in the read by ballot, its place kept for the passes below;
 *                        the visit's start and end cells counted (modasm.c:629-630,636-637); a visit the reference cannot do raises the error word
 *   mgRdnaSuffixKernel   the two count arrays of every tested mod suffix-summed (modasm.c:651-654), a workgroup per array
 *   mgRdnaAccumKernel    a workgroup per (tested mod, tile of MG_RD_TILE partner ordinals, share of the visits): the visited reads' hits streamed, a
 *                        lane per hit, count / min / max per partner ordinal in LDS (thousands of visits land on one (i, m): lanes of one wave hold
 *                        different hits of one read, so mostly different partners), flushed with one integer atomic per cell that was touched
 *   mgRdnaRuleKernel     a workgroup per tested mod over its cells: the rules of modasm.c:658-705 (mgRdnaLdRule, shared with the host loops);
 *                        nGood / nMod2 / nSplit reduced over the workgroup, nBadLD / nSplitLD of OTHER mods by atomicAdd
 *   mgRdnaEmitKernel     only when the "ZZ-TEST" lines are wanted: the cells that hold something, in partner order, placed by a workgroup scan
 * A partner universe larger than a tile is covered by more workgroups (blockIdx.y), each streaming the same hits and keeping its own ordinals: no
 * sort, no second path; the cost is one more read of the hits per 4096 partners.  Nothing of the set stays on the device between calls. */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_xfer.h"

#define MG_RD_NONE    0xffffffffu
#define MG_RD_TILE    4096           /* partner ordinals per workgroup: three words each, 48 KiB of LDS */
#define MG_RD_WAVES   4              /* waves per workgroup of 256 */

/* ---- -R ---- */

/* the hit number (from 0) of the need-th set bit of the wave's ballot, lane by lane: every lane returns it */
__device__ __forceinline__ U32 mgRdnaNthLane (U64 mask, bool q, U32 lane, U32 need)
{
  const U32 rank = (U32) __popcll (mask & (((U64) 1 << lane) - 1)) + 1;
  const U64 at = __ballot (q && rank == need);
  return (U32) __ffsll ((long long) at) - 1;
}

__global__ __launch_bounds__ (256)
void mgRdnaN200Kernel (const U32 *__restrict__ hit, const U64 *__restrict__ hitStart, U32 nReads, const U8 *__restrict__ qual, int *__restrict__ n200, int *__restrict__ m200)
{
  const U32 r = 1 + blockIdx.x * MG_RD_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r > nReads) return;
  const U64 h0 = hitStart[r];
  const U32 nHit = (U32) (hitStart[r + 1] - h0);
  U32 fwd = 0, back = 0, n = 0;
  for (U32 base = 0 ; base < nHit ; base += 64)
    { const U32 j = base + lane;
      const bool q = j < nHit && qual[hit[h0 + j] & MG_TOPMASK];
      const U64 mask = __ballot (q);
      const U32 c = (U32) __popcll (mask);
      if (n + c >= 200) { fwd = base + mgRdnaNthLane (mask, q, lane, 200 - n); break; }
      n += c;
    }
  if (fwd)                                                         /* from the back, never hit 0 (modasm.c:793: for (j = nHit ; --j ; )) */
    { n = 0;
      for (U32 base = 0 ; base + 1 < nHit ; base += 64)
        { const U32 o = base + lane;
          const bool v = o + 1 < nHit;
          const bool q = v && qual[hit[h0 + (nHit - 1 - o)] & MG_TOPMASK];
          const U64 mask = __ballot (q);
          const U32 c = (U32) __popcll (mask);
          if (n + c >= 200) { back = nHit - 1 - (base + mgRdnaNthLane (mask, q, lane, 200 - n)); break; }
          n += c;
        }
    }
  if (!lane) { n200[r] = (int) fwd; m200[r] = (int) back; }
}

static bool mgRdnaRoom (size_t bytes, size_t *freeOut)
{
  size_t freeB = 0;
  if (!mgDevFreeBytes (&freeB)) return false;
  if (freeOut) *freeOut = freeB;
  return bytes + ((size_t) 64 << 20) < freeB;
}

/* hQual[msMax + 1], v's hit lists: in; hN200[nReads + 1], hM200[nReads + 1]: out */
extern "C" int mgRdnaN200Device (const MgRsView *v, const U8 *hQual, int *hN200, int *hM200)
{
  const U32 nReads = v->nReads; const U64 totHit = v->totHit;
  if (!nReads) return 0;
  if (mgEnsureDevice ()) return -1;
  const size_t m = (size_t) v->msMax + 1;
  if (!mgRdnaRoom (m + (totHit + 1) * 4 + ((size_t) nReads + 3) * 16, 0)) return 1;
  MgDevScratch scratch ("modasm -R on the device");
  U8 *dQual; U32 *dHit; U64 *dStart; int *dN, *dM;
  if (scratch.get (&dQual, m) || scratch.get (&dHit, totHit + 1) || scratch.get (&dStart, (size_t) nReads + 3) || scratch.get (&dN, (size_t) nReads + 2) || scratch.get (&dM, (size_t) nReads + 2)) return -1;
  if (mgXferH2D (dQual, hQual, m) || mgXferH2D (dStart, v->hitStart, ((size_t) nReads + 2) * 8) || (totHit && mgXferH2D (dHit, v->hit, totHit * 4))) return -1;
  hipLaunchKernelGGL (mgRdnaN200Kernel, dim3 ((nReads + MG_RD_WAVES - 1) / MG_RD_WAVES), dim3 (256), 0, 0, dHit, dStart, nReads, dQual, dN, dM);
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (0)) { scratch.fail (); return -1; }
  if (mgXferD2H (hN200 + 1, dN + 1, (size_t) nReads * 4, MG_XFER_COPY) || mgXferD2H (hM200 + 1, dM + 1, (size_t) nReads * 4, MG_XFER_COPY)) return -1;
  return 0;
}

/* ---- -T ---- */

/* per hit its position in the read (the inclusive sum of dx: modasm.c:626) and its mod's partner ordinal (MG_RD_NONE: fails checkMod); a wave per read */
__global__ __launch_bounds__ (256)
void mgRdnaPosKernel (const U32 *__restrict__ hit, const unsigned short *__restrict__ dx, const U64 *__restrict__ hitStart, U32 nReads, const U32 *__restrict__ ordOf,
                      int *__restrict__ pos, U32 *__restrict__ hord)
{
  const U32 lane = threadIdx.x & 63;
  for (U64 r = 1 + (U64) blockIdx.x * MG_RD_WAVES + (threadIdx.x >> 6) ; r <= nReads ; r += (U64) gridDim.x * MG_RD_WAVES)
    { const U64 h0 = hitStart[r], h1 = hitStart[r + 1];
      U32 carry = 0;
      for (U64 base = h0 ; base < h1 ; base += 64)
        { const U64 h = base + lane;
          const U32 inc = mgWaveInclusiveSum (h < h1 ? (U32) dx[h] : 0u);
          if (h < h1) { pos[h] = (int) (carry + inc); hord[h] = ordOf[hit[h] & MG_TOPMASK]; }
          carry += (U32) __shfl ((int) inc, 63);
        }
    }
}

__device__ __forceinline__ void mgRdnaRaise (U32 *__restrict__ err, U32 code, U32 mod) { if (atomicCAS (&err[0], 0u, code) == 0u) err[1] = mod; }

/* E: cells per count array (the longest read's length + 1).  ext[2b], ext[2b + 1]: the extents of b's start and end arrays (arrayMax of modasm.c:649-654) */
__global__ __launch_bounds__ (256)
void mgRdnaVisitKernel (const U32 *__restrict__ tested, const U64 *__restrict__ invStart, const U32 *__restrict__ invSpace, const U32 *__restrict__ hit,
                        const U64 *__restrict__ hitStart, const int *__restrict__ len, const int *__restrict__ pos, int w, U32 E,
                        U32 *__restrict__ visitFirst, int *__restrict__ startArr, int *__restrict__ endArr, int *__restrict__ ext, U32 *__restrict__ err)
{
  const U32 b = blockIdx.x, i = tested[b], lane = threadIdx.x & 63;
  const U64 v1 = invStart[i + 1];
  for (U64 v = invStart[i] + (threadIdx.x >> 6) ; v < v1 ; v += MG_RD_WAVES)
    { const U32 r = invSpace[v];
      const U64 h0 = hitStart[r], h1 = hitStart[r + 1];
      U64 first = ~(U64) 0;
      for (U64 base = h0 ; base < h1 ; base += 64)
        { const U64 h = base + lane;
          const U64 mask = __ballot (h < h1 && (hit[h] & MG_TOPMASK) == i);
          if (mask) { first = base + (U64) (__ffsll ((long long) mask) - 1); break; }
        }
      if (lane) continue;
      U32 keep = MG_RD_NONE;
      if (first == ~(U64) 0) mgRdnaRaise (err, 3u, i);              /* the list names a read that does not hold the mod */
      else
        { const int x = pos[first], o = len[r] - x - w;
          if (o < 0 || x < 0 || (U32) x >= E || (U32) o >= E) mgRdnaRaise (err, 1u, i);      /* modasm.c:630,636 would write before the array */
          else
            { const bool fwd = (hit[first] & ~MG_TOPMASK) != 0;
              const int s = fwd ? x : o, e = fwd ? o : x;
              atomicAdd (&startArr[(size_t) b * E + s], 1); atomicAdd (&endArr[(size_t) b * E + e], 1);
              atomicMax (&ext[2 * b], s + 1); atomicMax (&ext[2 * b + 1], e + 1);
              keep = (U32) first;
            }
        }
      visitFirst[v] = keep;
    }
}

/* a[j] = a[j] + a[j + 1] + ... over the array's extent, 256 cells a step from the top; blockIdx.y: 0 the start arrays, 1 the end arrays */
__global__ __launch_bounds__ (256)
void mgRdnaSuffixKernel (int *__restrict__ startArr, int *__restrict__ endArr, const int *__restrict__ ext, U32 E)
{
  __shared__ U32 lds[4];
  int *a = (blockIdx.y ? endArr : startArr) + (size_t) blockIdx.x * E;
  U32 carry = 0;
  for (U32 top = (U32) ext[2 * blockIdx.x + blockIdx.y] ; top > 0 ; top = top > 256 ? top - 256 : 0)
    { const bool v = threadIdx.x < top;
      const U32 j = v ? top - 1 - threadIdx.x : 0;
      U32 tot;
      const U32 inc = mgBlockInclusive<256, MgSum> (v ? (U32) a[j] : 0u, lds, &tot);
      if (v) a[j] = (int) (carry + inc);
      carry += tot;
    }
}

__global__ __launch_bounds__ (256)
void mgRdnaAccumKernel (const U32 *__restrict__ tested, const U64 *__restrict__ invStart, const U32 *__restrict__ invSpace, const U32 *__restrict__ hit,
                        const U64 *__restrict__ hitStart, const int *__restrict__ pos, const U32 *__restrict__ hord, const U32 *__restrict__ visitFirst,
                        U32 nP, int *__restrict__ cCnt, int *__restrict__ cMin, int *__restrict__ cMax)
{
  __shared__ int sCnt[MG_RD_TILE], sMin[MG_RD_TILE], sMax[MG_RD_TILE];
  const U32 b = blockIdx.x, tile0 = blockIdx.y * MG_RD_TILE, i = tested[b], lane = threadIdx.x & 63;
  for (U32 o = threadIdx.x ; o < MG_RD_TILE ; o += 256) { sCnt[o] = 0; sMin[o] = 0x7fffffff; sMax[o] = (int) 0x80000000; }
  __syncthreads ();
  const U64 v1 = invStart[i + 1];
  for (U64 v = invStart[i] + (U64) blockIdx.z * MG_RD_WAVES + (threadIdx.x >> 6) ; v < v1 ; v += (U64) gridDim.z * MG_RD_WAVES)
    { const U32 f = visitFirst[v];
      if (f == MG_RD_NONE) continue;
      const U32 r = invSpace[v];
      const U64 h0 = hitStart[r], h1 = hitStart[r + 1];
      const int x = pos[f];
      const bool fwd = (hit[f] & ~MG_TOPMASK) != 0;
      for (U64 h = h0 + lane ; h < h1 ; h += 64)                      /* every other hit of the read, later occurrences of i itself among them */
        { const U32 o = hord[h] - tile0;
          if (h == f || o >= MG_RD_TILE) continue;                   /* (MG_RD_NONE - tile0 is no ordinal of a tile either) */
          const int d = fwd ? pos[h] - x : x - pos[h];
          atomicAdd (&sCnt[o], 1); atomicMin (&sMin[o], d); atomicMax (&sMax[o], d);
        }
    }
  __syncthreads ();
  for (U32 o = threadIdx.x ; o < MG_RD_TILE && tile0 + o < nP ; o += 256)
    if (sCnt[o])
      { const size_t c = (size_t) b * nP + tile0 + o;
        atomicAdd (&cCnt[c], sCnt[o]); atomicMin (&cMin[c], sMin[o]); atomicMax (&cMax[c], sMax[o]);
      }
}

struct MgRdnaCells { const U32 *tested, *partner; U32 nP, E; const int *cCnt, *cMin, *cMax, *startArr, *endArr, *ext; const unsigned short *depth; int run; };

__device__ __forceinline__ int mgRdnaCellRule (const MgRdnaCells &C, U32 b, U32 o, int n, MgLdCell *cell)
{
  const size_t c = (size_t) b * C.nP + o;
  cell->m = C.partner[o];
  return mgRdnaLdRule (n, C.cMin[c], C.cMax[c], C.startArr + (size_t) b * C.E, C.ext[2 * b], C.endArr + (size_t) b * C.E, C.ext[2 * b + 1], (int) C.depth[cell->m], C.run, cell);
}

/* res4[4b ..]: nGood, nMod2, nSplit of tested mod b, the cells it holds */
__global__ __launch_bounds__ (256)
void mgRdnaRuleKernel (MgRdnaCells C, int *__restrict__ res4, int *__restrict__ badLD, int *__restrict__ splitLD, U32 *__restrict__ err, unsigned long long *__restrict__ occ)
{
  __shared__ U32 lds[4];
  const U32 b = blockIdx.x, i = C.tested[b];
  U32 nGood = 0, nMod2 = 0, nSplit = 0, nCells = 0, badI = 0, seen = 0;
  for (U32 o = threadIdx.x ; o < C.nP ; o += 256)
    { const int n = C.cCnt[(size_t) b * C.nP + o];
      if (!n) continue;
      MgLdCell cell;
      ++nCells; seen += (U32) n;
      if (mgRdnaCellRule (C, b, o, n, &cell)) { mgRdnaRaise (err, 2u, i); continue; }
      nGood += (cell.flags & MG_LD_GOOD) != 0; nMod2 += (cell.flags & MG_LD_MOD2) != 0; badI += (cell.flags & MG_LD_BAD_I) != 0;
      if (cell.flags & MG_LD_SPLIT) { ++nSplit; atomicAdd (&splitLD[cell.m], 1); }
      if (cell.flags & MG_LD_BAD_M) atomicAdd (&badLD[cell.m], 1);
    }
  nGood = mgBlockReduce<256, MgSum> (nGood, lds); nMod2 = mgBlockReduce<256, MgSum> (nMod2, lds); nSplit = mgBlockReduce<256, MgSum> (nSplit, lds);
  nCells = mgBlockReduce<256, MgSum> (nCells, lds); badI = mgBlockReduce<256, MgSum> (badI, lds); seen = mgBlockReduce<256, MgSum> (seen, lds);
  if (threadIdx.x) return;
  res4[4 * b] = (int) nGood; res4[4 * b + 1] = (int) nMod2; res4[4 * b + 2] = (int) nSplit; res4[4 * b + 3] = (int) nCells;
  if (badI) atomicAdd (&badLD[i], (int) badI);
  if (seen) atomicAdd (occ, (unsigned long long) seen);
}

/* the cells of tested mod b that hold something, partner ascending, from out[cellAt[b]] on */
__global__ __launch_bounds__ (256)
void mgRdnaEmitKernel (MgRdnaCells C, const U32 *__restrict__ cellAt, MgLdCell *__restrict__ out)
{
  __shared__ U32 lds[4];
  const U32 b = blockIdx.x;
  U32 at = cellAt[b];
  for (U32 base = 0 ; base < C.nP ; base += 256)
    { const U32 o = base + threadIdx.x;
      const int n = o < C.nP ? C.cCnt[(size_t) b * C.nP + o] : 0;
      U32 tot;
      const U32 inc = mgBlockInclusive<256, MgSum> (n ? 1u : 0u, lds, &tot);
      if (n) { MgLdCell cell; if (!mgRdnaCellRule (C, b, o, n, &cell)) out[at + inc - 1] = cell; }
      at += tot;
    }
}

extern "C" int mgRdnaTestModsDevice (const MgRsView *S, const U32 *tested, U32 nTested, const U32 *partner, U32 nPartner, U32 batch, int wantCells,
                                     int *res3, int *badLD, int *splitLD, U64 *cellStart, MgLdCell **cells, U64 diag[4], U32 grid[4], U32 *badMod)
{
  if (cells) *cells = 0;
  if (cellStart) cellStart[0] = 0;
  if (!nTested) return 0;
  if (mgEnsureDevice ()) return -1;
  hipStream_t st = 0;
  const size_t m = (size_t) S->msMax + 1, nR = S->nReads, nInv = (size_t) S->invStart[m];
  int maxLen = 0;
  for (U32 r = 1 ; r <= S->nReads ; ++r) if (S->len[r] > maxLen) maxLen = S->len[r];
  if (maxLen >= 0x7f000000) return 1;                               /* (the cells' idle values are beyond every distance) */
  const U32 E = (U32) maxLen + 1, nP = nPartner, nTiles = (nP + MG_RD_TILE - 1) / MG_RD_TILE;
  grid[0] = nTiles; grid[3] = E;
  const size_t fixed = m * 15 + (nR + 3) * 12 + (S->totHit + 1) * 14 + (m + 2) * 8 + (nInv + 1) * 8 + ((size_t) nTested + nP) * 4 + 4096;
  const size_t perMod = (size_t) nP * 12 + (size_t) E * 8 + 64;
  size_t freeB = 0;
  if (!mgRdnaRoom (fixed + perMod, &freeB)) return 1;
  U64 nb = batch;
  if (!nb)
    { size_t budget = (freeB - fixed - ((size_t) 64 << 20)) / 2;
      if (budget > ((size_t) 2 << 30)) budget = (size_t) 2 << 30;
      nb = budget / perMod;
    }
  if (nb > nTested) nb = nTested;
  while (nb > 1 && (nb * nP >= 0x7fffffffull || nb * E >= 0x7fffffffull)) nb /= 2;
  if (nb < 1) nb = 1;
  if (!mgRdnaRoom (fixed + nb * perMod, 0)) return 1;

  MgDevScratch scratch ("modasm -T on the device");
  unsigned short *dDepth, *dDx; U32 *dHit, *dOrdOf, *dHord, *dInvSpace, *dVisit, *dTested, *dPartner, *dErr, *dCellAt; U64 *dStart, *dInvStart; int *dLen, *dPos;
  int *dCnt, *dMin, *dMax, *dSA, *dEA, *dExt, *dRes, *dBadLD, *dSplitLD; unsigned long long *dOcc;
  if (scratch.get (&dDepth, m) || scratch.get (&dOrdOf, m) || scratch.get (&dBadLD, m) || scratch.get (&dSplitLD, m) || scratch.get (&dStart, nR + 3) || scratch.get (&dLen, nR + 2)
      || scratch.get (&dHit, S->totHit + 1) || scratch.get (&dDx, S->totHit + 1) || scratch.get (&dPos, S->totHit + 1) || scratch.get (&dHord, S->totHit + 1)
      || scratch.get (&dInvStart, m + 2) || scratch.get (&dInvSpace, nInv + 1) || scratch.get (&dVisit, nInv + 1) || scratch.get (&dTested, (size_t) nTested) || scratch.get (&dPartner, (size_t) nP + 1)
      || scratch.get (&dErr, 2) || scratch.get (&dOcc, 1) || scratch.get (&dCellAt, (size_t) nb) || scratch.get (&dExt, 2 * (size_t) nb) || scratch.get (&dRes, 4 * (size_t) nb)
      || scratch.get (&dCnt, (size_t) nb * nP + 1) || scratch.get (&dMin, (size_t) nb * nP + 1) || scratch.get (&dMax, (size_t) nb * nP + 1)
      || scratch.get (&dSA, (size_t) nb * E) || scratch.get (&dEA, (size_t) nb * E)) return -1;
  /* the partner ordinal of every mod */
  U32 *ordOf = (U32 *) malloc (m * 4);
  if (!ordOf) { mgSetError ("modasm -T on the device: out of memory"); return -1; }
  memset (ordOf, 0xff, m * 4);
  for (U32 o = 0 ; o < nP ; ++o) ordOf[partner[o]] = o;
  int bad = hipMemsetAsync (dBadLD, 0, m * 4, st) || hipMemsetAsync (dSplitLD, 0, m * 4, st) || hipMemsetAsync (dErr, 0, 8, st) || hipMemsetAsync (dOcc, 0, 8, st) || hipDeviceSynchronize ();
  if (bad) { free (ordOf); scratch.fail (); return -1; }
  bad = mgXferH2D (dOrdOf, ordOf, m * 4) || mgXferH2D (dDepth, S->depth, m * 2) || mgXferH2D (dStart, S->hitStart, (nR + 2) * 8) || mgXferH2D (dLen, S->len, (nR + 1) * 4)
        || (S->totHit && (mgXferH2D (dHit, S->hit, S->totHit * 4) || mgXferH2D (dDx, S->dx, S->totHit * 2))) || mgXferH2D (dInvStart, S->invStart, (m + 1) * 8)
        || (nInv && mgXferH2D (dInvSpace, S->invSpace, nInv * 4)) || mgXferH2D (dTested, tested, (size_t) nTested * 4) || (nP && mgXferH2D (dPartner, partner, (size_t) nP * 4));
  free (ordOf);
  if (bad) return -1;
  if (nR) hipLaunchKernelGGL (mgRdnaPosKernel, dim3 (mgGrid (nR, MG_RD_WAVES, 8192)), dim3 (256), 0, st, dHit, dDx, dStart, S->nReads, dOrdOf, dPos, dHord);

  MgLdCell *hCells = 0; U64 nCells = 0, capCells = 0;
  int *hRes = (int *) malloc ((size_t) nb * 16), *hExt = (int *) malloc ((size_t) nb * 8); U32 *hAt = (U32 *) malloc ((size_t) nb * 4);
  int nBig[2] = { 0, 0 };
  int rc = hRes && hAt && hExt ? 0 : -1;
  if (rc) mgSetError ("modasm -T on the device: out of memory");
  for (U64 t0 = 0 ; t0 < nTested && !rc ; t0 += nb)
    { const U32 n = (U32) (nTested - t0 < nb ? nTested - t0 : nb);
      U32 share = 1;                                                /* visits of one tested mod over several workgroups when the batch alone does not fill the device */
      while (share < 16 && (U64) n * nTiles * share < 1024) share *= 2;
      if (!grid[1] || share < grid[1]) grid[1] = share;
      if (share > grid[2]) grid[2] = share;
      if (hipMemsetAsync (dCnt, 0, (size_t) n * nP * 4 + 4, st) || hipMemsetAsync (dMin, 0x7f, (size_t) n * nP * 4 + 4, st) || hipMemsetAsync (dMax, 0x80, (size_t) n * nP * 4 + 4, st)
          || hipMemsetAsync (dSA, 0, (size_t) n * E * 4, st) || hipMemsetAsync (dEA, 0, (size_t) n * E * 4, st) || hipMemsetAsync (dExt, 0, (size_t) n * 8, st))
        { scratch.fail (); rc = -1; break; }
      MgRdnaCells C;
      C.tested = dTested + t0; C.partner = dPartner; C.nP = nP; C.E = E; C.cCnt = dCnt; C.cMin = dMin; C.cMax = dMax; C.startArr = dSA; C.endArr = dEA; C.ext = dExt; C.depth = dDepth; C.run = S->run;
      hipLaunchKernelGGL (mgRdnaVisitKernel, dim3 (n), dim3 (256), 0, st, dTested + t0, dInvStart, dInvSpace, dHit, dStart, dLen, dPos, S->w, E, dVisit, dSA, dEA, dExt, dErr);
      hipLaunchKernelGGL (mgRdnaSuffixKernel, dim3 (n, 2), dim3 (256), 0, st, dSA, dEA, dExt, E);
      if (nP)
        hipLaunchKernelGGL (mgRdnaAccumKernel, dim3 (n, nTiles, share), dim3 (256), 0, st, dTested + t0, dInvStart, dInvSpace, dHit, dStart, dPos, dHord, dVisit, nP, dCnt, dMin, dMax);
      hipLaunchKernelGGL (mgRdnaRuleKernel, dim3 (n), dim3 (256), 0, st, C, dRes, dBadLD, dSplitLD, dErr, dOcc);
      U32 err[2] = { 0, 0 };
      if (hipGetLastError () != hipSuccess || hipMemcpyAsync (hRes, dRes, (size_t) n * 16, hipMemcpyDeviceToHost, st) || hipMemcpyAsync (err, dErr, 8, hipMemcpyDeviceToHost, st)
          || hipMemcpyAsync (hExt, dExt, (size_t) n * 8, hipMemcpyDeviceToHost, st) || hipStreamSynchronize (st))
        { scratch.fail (); rc = -1; break; }
      if (err[0]) { if (badMod) *badMod = err[1]; rc = -2; break; }
      for (U32 b = 0 ; b < n && rc != -3 ; ++b)                       /* the second tested mod whose start (or end) array passes MG_RDNA_CLEARED cells: the reference reads stale ones */
        for (int y = 0 ; y < 2 ; ++y)
          if (hExt[2 * b + y] > MG_RDNA_CLEARED && ++nBig[y] > 1) { if (badMod) *badMod = tested[t0 + b]; rc = -3; break; }
      if (rc) break;
      ++diag[0];
      U64 inBatch = 0;
      for (U32 b = 0 ; b < n ; ++b)
        { res3[3 * (t0 + b)] = hRes[4 * b]; res3[3 * (t0 + b) + 1] = hRes[4 * b + 1]; res3[3 * (t0 + b) + 2] = hRes[4 * b + 2];
          hAt[b] = (U32) inBatch; inBatch += (U64) hRes[4 * b + 3];
          if (cellStart) cellStart[t0 + b + 1] = nCells + inBatch;
        }
      if (!wantCells || !inBatch) { nCells += inBatch; continue; }
      if (nCells + inBatch > capCells)
        { capCells = (nCells + inBatch) * 2; MgLdCell *q = (MgLdCell *) realloc (hCells, capCells * sizeof (MgLdCell));
          if (!q) { mgSetError ("modasm -T on the device: out of memory"); rc = -1; break; }
          hCells = q;
        }
      MgLdCell *dCells = 0;
      if (hipMalloc ((void **) &dCells, inBatch * sizeof (MgLdCell)) != hipSuccess) { scratch.fail (); rc = -1; break; }
      if (hipMemcpyAsync (dCellAt, hAt, (size_t) n * 4, hipMemcpyHostToDevice, st) != hipSuccess) { (void) hipFree (dCells); scratch.fail (); rc = -1; break; }
      hipLaunchKernelGGL (mgRdnaEmitKernel, dim3 (n), dim3 (256), 0, st, C, dCellAt, dCells);
      if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st)) { (void) hipFree (dCells); scratch.fail (); rc = -1; break; }
      const int x = mgXferD2H (hCells + nCells, dCells, inBatch * sizeof (MgLdCell), MG_XFER_COPY);
      (void) hipFree (dCells);
      if (x) { rc = -1; break; }
      nCells += inBatch;
    }
  unsigned long long occ = 0;
  if (!rc && (mgXferD2H (badLD, dBadLD, m * 4, MG_XFER_COPY) || mgXferD2H (splitLD, dSplitLD, m * 4, MG_XFER_COPY) || hipMemcpy (&occ, dOcc, 8, hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
  free (hRes); free (hAt); free (hExt);
  if (rc) { free (hCells); return rc; }
  diag[3] = occ;
  if (cells) *cells = hCells; else free (hCells);
  return 0;
}
