/* mg_rsdev.hip — the device side of modasm's read set: the end of the ingest and the -C and -P passes.  All three
 * group hits by mod with the stable sort of mg_devsort.hip and turn counts into places with its scan.
 *
 * Ingest: what readsetFileRead + invBuild (modasm.c:151-191,258-287) leave per MOD.  Per batch the hit lists are made by mg_chain.hip
 * (mgReadsetSeedsDevice); the hits per mod are counted THERE into an array that lives here across the batches of a file (rounds 1-4:
 * copied back and folded into ms->depth by a host loop over every mod, per batch).  At the end of the file: depth[] = the counts
 * saturated at 65 535 (modasm.c:174); the inverse lists -- for every mod that was hit and did not saturate, the reads that hit it, in read
 * order (modasm.c:266,278) -- are a stable sort of the hits' read numbers by mod, hits on saturated mods keyed past the last mod so that
 * they fall off the end; invStart[] is the exclusive scan of the lists' lengths; a read's copy-class tallies (modasm.c:276-277) are a
 * lane per read.
 * The arrays of MgReadsetDev live from a file's first batch to its end; what a call needs besides them is its MgDevScratch's.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <mutex>
#include <unordered_map>
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_xfer.h"
#include "mg_devsort.h"

struct MgReadsetDev { U32 *depth = 0; size_t cap = 0; U32 *hitAll = 0; U64 hitLen = 0, hitCap = 0; bool hitsKept = true; };      /* hitAll: the file's hit lists so far, kept on the device for the inverse lists (given up, and uploaded at the end instead, if the device has no room) */
static std::mutex gRsLock;
static std::unordered_map<const void *, MgReadsetDev> gRsDev;

extern "C" void mgReadsetDevForget (const void *rs)
{ std::lock_guard<std::mutex> g (gRsLock); auto it = gRsDev.find (rs); if (it != gRsDev.end ()) { (void) hipFree (it->second.depth); (void) hipFree (it->second.hitAll); gRsDev.erase (it); } }

/* the per-mod hit counts of the file that follows: device U32[msMax + 2], zero (modasm.c:158) */
extern "C" MgStatus mgReadsetDevBegin (const void *rs, U32 msMax, U32 **dDepth)
{
  std::lock_guard<std::mutex> g (gRsLock);
  MgReadsetDev &d = gRsDev[rs];
  const size_t want = (size_t) msMax + 2;
  if (d.cap < want) { (void) hipFree (d.depth); d.depth = 0; d.cap = 0; MG_HIP (hipMalloc ((void **) &d.depth, want * 4)); d.cap = want; }
  MG_HIP (hipMemset (d.depth, 0, want * 4));
  d.hitLen = 0; d.hitsKept = true;
  *dDepth = d.depth;
  return MG_OK;
}

/* a batch's hit list (device, n words) behind the file's so far */
extern "C" void mgReadsetDevAppendHits (const void *rs, const U32 *dHit, U64 n)
{
  std::lock_guard<std::mutex> g (gRsLock);
  auto it = gRsDev.find (rs); if (it == gRsDev.end ()) return;
  MgReadsetDev &d = it->second;
  if (!d.hitsKept || !n) return;
  if (d.hitLen + n > d.hitCap)
    { const U64 cap = (d.hitLen + n) + (d.hitLen ? (d.hitLen + n) / 2 : 0) + 1024;      /* (a file that is one batch gets what it needs; one of many batches grows by halves) */
      U32 *q = 0;
      if (hipMalloc ((void **) &q, cap * 4) != hipSuccess || (d.hitLen && hipMemcpy (q, d.hitAll, d.hitLen * 4, hipMemcpyDeviceToDevice) != hipSuccess))
        { (void) hipGetLastError (); (void) hipFree (q); (void) hipFree (d.hitAll); d.hitAll = 0; d.hitCap = d.hitLen = 0; d.hitsKept = false; return; }
      (void) hipFree (d.hitAll); d.hitAll = q; d.hitCap = cap;
    }
  if (hipMemcpy (d.hitAll + d.hitLen, dHit, n * 4, hipMemcpyDeviceToDevice) != hipSuccess) { (void) hipGetLastError (); d.hitsKept = false; return; }
  d.hitLen += n;
}

__global__ void mgRsCountKernel (const U32 *__restrict__ depth32, U32 msMax, U32 *__restrict__ cnt, unsigned short *__restrict__ depth16)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= (U64) msMax + 1 ; i += (U64) gridDim.x * blockDim.x)
    { const U32 dp = (i >= 1 && i <= msMax) ? depth32[i] : 0u;
      cnt[i] = (dp && dp < 0xffffu) ? dp : 0u;                       /* a list only for a mod that was hit and did not saturate (modasm.c:266) */
      if (i <= msMax) depth16[i] = (unsigned short) (dp > 0xffffu ? 0xffffu : dp);
    }
}
__global__ void mgRsWidenKernel (const U32 *__restrict__ a, U64 n, U64 *__restrict__ out)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x) out[i] = a[i]; }
/* the read whose hitStart range holds hit h: the last r in 1 .. nReads with hitStart[r] <= h (an empty read never is) */
__device__ __forceinline__ U32 mgRsReadOf (const U64 *__restrict__ hitStart, U32 nReads, U64 h)
{
  U32 lo = 1, hi = nReads;
  while (lo < hi) { const U32 mid = lo + (hi - lo + 1) / 2; if (hitStart[mid] <= h) lo = mid; else hi = mid - 1; }
  return lo;
}
/* per hit: key = its mod (past the last mod if that one saturated), value = its read: the one whose hitStart range holds it (reads from 1) */
__global__ void mgRsKeyValKernel (const U32 *__restrict__ hit, U64 nHit, const U64 *__restrict__ hitStart, U32 nReads, const U32 *__restrict__ depth32, U32 msMax,
                                  U32 *__restrict__ key, U32 *__restrict__ val)
{
  for (U64 h = (U64) blockIdx.x * blockDim.x + threadIdx.x ; h < nHit ; h += (U64) gridDim.x * blockDim.x)
    { const U32 y = hit[h] & MG_TOPMASK;
      key[h] = depth32[y] < 0xffffu ? y : msMax + 1;
      val[h] = mgRsReadOf (hitStart, nReads, h);
    }
}
__global__ __launch_bounds__ (256)
void mgRsCopyTallyKernel (const U32 *__restrict__ hit, const U64 *__restrict__ hitStart, U32 nReads, const U8 *__restrict__ info, int4 *__restrict__ nCopy)
{
  const U32 r = 1 + blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nReads) return;
  int c[4] = { 0, 0, 0, 0 };
  const U64 h0 = hitStart[r], h1 = hitStart[r + 1];
  for (U64 h = h0 ; h < h1 ; h += 8)
    { U32 cl[8];
#pragma unroll
      for (int j = 0 ; j < 8 ; ++j) cl[j] = h + j < h1 ? (U32) info[hit[h + j] & MG_TOPMASK] & 3u : 4u;      /* eight gathers in flight */
#pragma unroll
      for (int j = 0 ; j < 8 ; ++j) { c[0] += cl[j] == 0; c[1] += cl[j] == 1; c[2] += cl[j] == 2; c[3] += cl[j] == 3; }
    }
  nCopy[r] = make_int4 (c[0], c[1], c[2], c[3]);
}

/* v's hit lists and info[]: in.  hDepth16[msMax + 1], hInvStart[msMax + 2], *hInvSpace (malloc ()ed here, the lists' total length words),
   hNCopy[(nReads + 1) * 4]: out.  totHit < 2^32 - 1. */
extern "C" MgStatus mgReadsetFinishDevice (const void *rs, Modset *ms, const MgRsView *v, U16 *hDepth16, U64 *hInvStart, U32 **hInvSpace, int *hNCopy)
{
  const U32 msMax = v->msMax, nReads = v->nReads; const U64 totHit = v->totHit;
  *hInvSpace = 0;
  MgReadsetDev d;
  bool kept = false;
  { std::lock_guard<std::mutex> g (gRsLock); auto it = gRsDev.find (rs); if (it == gRsDev.end ()) { mgSetError ("mgReadsetFinishDevice: no read set in progress"); return MG_ERR_ARG; }
    d = it->second;
    kept = d.hitsKept && d.hitAll && d.hitLen == totHit && totHit;      /* the lists are on the device already: no upload */
    if (kept) { it->second.hitAll = 0; it->second.hitCap = it->second.hitLen = 0; }      /* (this call owns them now, and frees them) */
    else { (void) hipFree (it->second.hitAll); it->second.hitAll = 0; it->second.hitCap = it->second.hitLen = 0; }
  }
  hipStream_t st = 0;
  const size_t m = (size_t) msMax + 1;
  MgDevScratch scratch ("read set on the device");
  if (kept) scratch.adopt (d.hitAll);
  U32 *dHit = kept ? d.hitAll : 0, *dCnt, *dKey, *dVal, *dSorted = 0; U64 *dStart, *dInv64; U8 *dInfo; unsigned short *dD16; int4 *dNc;
  MgStatus s;
  if (scratch.get (&dCnt, m + 2) || scratch.get (&dD16, m + 1) || scratch.get (&dInv64, m + 2) || scratch.get (&dInfo, m) || scratch.get (&dStart, (size_t) nReads + 3)
      || scratch.get (&dNc, (size_t) nReads + 2) || (!kept && scratch.get (&dHit, totHit + 1)) || scratch.get (&dKey, totHit + 1) || scratch.get (&dVal, totHit + 1)) return MG_ERR_HIP;
  if (hipDeviceSynchronize ()) return scratch.fail ();
  if ((s = mgXferH2DSparse (dInfo, v->info, m)) || (s = mgXferH2D (dStart, v->hitStart, ((size_t) nReads + 2) * 8)) || (totHit && !kept && (s = mgXferH2D (dHit, v->hit, totHit * 4)))) return s;
  hipLaunchKernelGGL (mgRsCountKernel, dim3 (2048), dim3 (256), 0, st, d.depth, msMax, dCnt, dD16);
  if ((s = mgExclusiveScan (scratch, dCnt, dCnt, m + 1, st))) return s;      /* dCnt[i] = first place of mod i's list; [msMax + 1] = the lists' total */
  hipLaunchKernelGGL (mgRsWidenKernel, dim3 (2048), dim3 (256), 0, st, dCnt, (U64) m + 1, dInv64);
  if (nReads) hipLaunchKernelGGL (mgRsCopyTallyKernel, dim3 ((nReads + 255) / 256), dim3 (256), 0, st, dHit, dStart, nReads, dInfo, dNc);
  U32 listed = 0;
  if (hipMemcpyAsync (&listed, dCnt + m, 4, hipMemcpyDeviceToHost, st) || hipStreamSynchronize (st)) return scratch.fail ();
  if (totHit)
    { hipLaunchKernelGGL (mgRsKeyValKernel, dim3 (4096), dim3 (256), 0, st, dHit, totHit, dStart, nReads, d.depth, msMax, dKey, dVal);
      if ((s = mgRefStableSort (scratch, dKey, dVal, (U32) totHit, mgKeyBits ((U64) msMax + 1), &dSorted, st))) return s;
    }
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st)) return scratch.fail ();
  U32 *inv = (U32 *) mgAllocBig (((size_t) listed ? listed : 1) * 4);
  if (!inv) return MG_ERR_NOMEM;
  if ((s = mgXferD2H (hDepth16, dD16, m * 2, MG_XFER_COPY)) || (s = mgXferD2H (hInvStart, dInv64, (m + 1) * 8, MG_XFER_COPY))
      || (listed && (s = mgXferD2H (inv, dSorted, (size_t) listed * 4, MG_XFER_COPY)))
      || (nReads && (s = mgXferD2H (hNCopy + 4, dNc + 1, (size_t) nReads * sizeof (int4), MG_XFER_COPY)))
      || (s = mgModsetAdoptDepthDevice (ms, (const U16 *) dD16)))      /* the device table keeps up with the depth[] just mirrored (no rebuild on its next use) */
    { free (inv); return s; }
  *hInvSpace = inv;
  return MG_OK;
}

/* ---------------------------------------------------------------------------------------- */
/* modasm -C and -P (cleanMods, modasm.c:514-555; readProperties, modasm.c:912-952) for a read set that is on the host: both ask how
 * often a mod occurs in ONE read.  The reference answers with an array of ms->max + 1 entries that it clears per read; here the hits'
 * ordinals are sorted stably by mod (mgRefStableSort, no key past the last mod: saturated mods count), which leaves the hits of one
 * mod in read order -- the occurrences of a mod in one read are neighbours.  The flags of -C are OR-ed into the 32-bit words of info[]
 * with integer atomics (a result that does not depend on the order); the tallies of -P are integer atomicAdd per read.  Nothing of
 * the read set stays on the device: a call uploads what it reads. */

__device__ __forceinline__ void mgRsInfoOr (U32 *__restrict__ info32, U32 y, U32 flag) { atomicOr (&info32[y >> 2], flag << (8u * (y & 3u))); }

/* per hit its mod and its read (for all nHit hits); for the nClean first -- the hits of reads 1 .. nReads - 1: modasm.c:522-523 starts its
   Read pointer at entry 0 and so never looks at the last read -- the internal and the minor-variant rule (modasm.c:533-538) */
__global__ __launch_bounds__ (256)
void mgRsCleanNeighbourKernel (const U32 *__restrict__ hit, const unsigned short *__restrict__ dx, U64 nHit, U64 nClean, const U64 *__restrict__ hitStart, U32 nReads,
                               const unsigned short *__restrict__ depth, int w, U32 *__restrict__ info32, U32 *__restrict__ key, U32 *__restrict__ rd)
{
  for (U64 h = (U64) blockIdx.x * blockDim.x + threadIdx.x ; h < nHit ; h += (U64) gridDim.x * blockDim.x)
    { const U32 y = hit[h] & MG_TOPMASK;
      const U32 r = mgRsReadOf (hitStart, nReads, h);
      key[h] = y; rd[h] = r;
      if (h >= nClean || h == hitStart[r]) continue;                 /* the rules are about a hit and the one before it in the read */
      if (h + 1 < hitStart[r + 1] && (int) dx[h] < w && (int) dx[h + 1] < w) mgRsInfoOr (info32, y, MS_INTERNAL);
      const U32 p = hit[h - 1] & MG_TOPMASK;
      const int lastDepth = depth[p], thisDepth = depth[y];
      if (lastDepth > 2 * thisDepth) mgRsInfoOr (info32, y, MS_MINOR);
      if (thisDepth > 2 * lastDepth) mgRsInfoOr (info32, p, MS_MINOR);
    }
}
/* sorted[0 .. n): hit ordinals, by mod, in hit order inside a mod: a mod is in one read twice when two neighbours share mod and read */
__global__ __launch_bounds__ (256)
void mgRsCleanRepeatKernel (const U32 *__restrict__ sorted, U64 n, const U32 *__restrict__ key, const U32 *__restrict__ rd, U32 *__restrict__ info32)
{
  for (U64 i = 1 + (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 a = sorted[i - 1], b = sorted[i];
      if (key[a] == key[b] && rd[a] == rd[b]) mgRsInfoOr (info32, key[b], MS_REPEAT);
    }
}
/* modasm.c:545-550: entries 0 .. max; counts[3] = repeat, internal, minor */
__global__ __launch_bounds__ (256)
void mgRsCleanCountKernel (const U8 *__restrict__ info, U32 max, U32 *__restrict__ counts)
{
  __shared__ U32 lds[4];
  U32 c[3] = { 0, 0, 0 };
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= max ; i += (U64) gridDim.x * blockDim.x)
    { const U32 f = info[i]; c[0] += (f & MS_REPEAT) != 0; c[1] += (f & MS_INTERNAL) != 0; c[2] += (f & MS_MINOR) != 0; }
  for (int j = 0 ; j < 3 ; ++j)
    { const U32 s = mgBlockReduce<256, MgSum> (c[j], lds);
      if (!threadIdx.x && s) atomicAdd (&counts[j], s);
    }
}

static size_t mgRsSortScratchWords (U64 n) { return (size_t) 256 * ((n + MG_RSORT_TILE - 1) / MG_RSORT_TILE + 1); }      /* the histogram of a sort of n elements */
/* is there room for `bytes` of arrays next to what a stable sort of n elements with keys takes itself (two value and two key arrays, its histogram)? */
static bool mgRsRoom (size_t bytes, U64 n)
{
  size_t freeB = 0;
  return mgDevFreeBytes (&freeB) && bytes + (size_t) n * 16 + mgRsSortScratchWords (n) * 4 + ((size_t) 64 << 20) < freeB;
}

/* v's hit lists, distances and depth[]: in; hInfo[msMax + 1]: in and out; hNCopy[(nReads + 1) * 4], counts[3]: out.  totHit < 2^32 - 16.
   0 = done, 1 = the device has no room (nothing was changed: the caller takes its host loops), -1 = failed */
extern "C" int mgReadsetCleanDevice (const MgRsView *v, U8 *hInfo, int *hNCopy, U32 counts[3])
{
  if (mgEnsureDevice ()) return -1;
  const U32 msMax = v->msMax, nReads = v->nReads; const U64 totHit = v->totHit;
  hipStream_t st = 0;
  const size_t m = (size_t) msMax + 1, m4 = (m + 3) / 4 * 4;
  const U64 nClean = nReads > 1 ? v->hitStart[nReads] : 0;          /* the hits of reads 1 .. nReads - 1 */
  const size_t scanTiles = mgScanScratchWords (mgRsSortScratchWords (totHit));
  const size_t bytes = m4 + m * 2 + ((size_t) nReads + 3) * 8 + ((size_t) nReads + 2) * sizeof (int4) + (totHit + 1) * 14 + scanTiles * 4 + 64;
  if (!mgRsRoom (bytes, nClean)) return 1;
  MgDevScratch scratch ("modasm -C on the device");
  U32 *dHit, *dKey, *dRd, *dSorted, *dCounts; unsigned short *dDx, *dD16; U64 *dStart; U8 *dInfo; int4 *dNc;
  if (scratch.get (&dCounts, 4) || scratch.get (&dD16, m) || scratch.get (&dInfo, m4) || scratch.get (&dStart, (size_t) nReads + 3) || scratch.get (&dNc, (size_t) nReads + 2)
      || scratch.get (&dHit, totHit + 1) || scratch.get (&dDx, totHit + 1) || scratch.get (&dKey, totHit + 1) || scratch.get (&dRd, totHit + 1)) return -1;
  if (hipMemset (dCounts, 0, 16) || hipMemset (dInfo + (m4 - 4), 0, 4) || hipDeviceSynchronize ()) { scratch.fail (); return -1; }
  if (mgXferH2D (dInfo, hInfo, m) || mgXferH2D (dD16, v->depth, m * 2) || mgXferH2D (dStart, v->hitStart, ((size_t) nReads + 2) * 8)
      || (totHit && (mgXferH2D (dHit, v->hit, totHit * 4) || mgXferH2D (dDx, v->dx, totHit * 2)))) return -1;
  if (totHit)
    hipLaunchKernelGGL (mgRsCleanNeighbourKernel, dim3 (4096), dim3 (256), 0, st, dHit, dDx, totHit, nClean, dStart, nReads, dD16, v->w, (U32 *) dInfo, dKey, dRd);
  if (nClean > 1)
    { if (mgRefStableSort (scratch, dKey, 0, (U32) nClean, mgKeyBits (msMax), &dSorted, st)) return -1;
      hipLaunchKernelGGL (mgRsCleanRepeatKernel, dim3 (4096), dim3 (256), 0, st, dSorted, nClean, dKey, dRd, (U32 *) dInfo);
    }
  hipLaunchKernelGGL (mgRsCleanCountKernel, dim3 (1024), dim3 (256), 0, st, dInfo, msMax, dCounts);
  if (nReads) hipLaunchKernelGGL (mgRsCopyTallyKernel, dim3 ((nReads + 255) / 256), dim3 (256), 0, st, dHit, dStart, nReads, dInfo, dNc);      /* invBuild's nCopy[] (modasm.c:552,273-277) */
  if (hipGetLastError () != hipSuccess || hipMemcpyAsync (counts, dCounts, 12, hipMemcpyDeviceToHost, st) || hipStreamSynchronize (st)) { scratch.fail (); return -1; }
  if (mgXferD2H (hInfo, dInfo, m, MG_XFER_COPY) || (nReads && mgXferD2H (hNCopy + 4, dNc + 1, (size_t) nReads * sizeof (int4), MG_XFER_COPY))) return -1;
  return 0;
}

/* invBuild's nCopy[] alone (modasm.c:273-277), after a pass that changed copy classes and nothing else (-rb, -T): hNCopy[(nReads + 1) * 4] out.
   0 = done, 1 = the device has no room, -1 = failed */
extern "C" int mgReadsetCopyTallyDevice (const MgRsView *v, const U8 *hInfo, int *hNCopy)
{
  const U32 nReads = v->nReads; const U64 totHit = v->totHit;
  if (!nReads) return 0;
  if (mgEnsureDevice ()) return -1;
  const size_t m = (size_t) v->msMax + 1;
  if (!mgRsRoom (m + ((size_t) nReads + 3) * 8 + ((size_t) nReads + 2) * sizeof (int4) + (totHit + 1) * 4, 0)) return 1;
  MgDevScratch scratch ("read set copy tallies on the device");
  U32 *dHit; U64 *dStart; U8 *dInfo; int4 *dNc;
  if (scratch.get (&dInfo, m) || scratch.get (&dStart, (size_t) nReads + 3) || scratch.get (&dNc, (size_t) nReads + 2) || scratch.get (&dHit, totHit + 1)) return -1;
  if (mgXferH2D (dInfo, hInfo, m) || mgXferH2D (dStart, v->hitStart, ((size_t) nReads + 2) * 8) || (totHit && mgXferH2D (dHit, v->hit, totHit * 4))) return -1;
  hipLaunchKernelGGL (mgRsCopyTallyKernel, dim3 ((nReads + 255) / 256), dim3 (256), 0, 0, dHit, dStart, nReads, dInfo, dNc);
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (0)) { scratch.fail (); return -1; }
  if (mgXferD2H (hNCopy + 4, dNc + 1, (size_t) nReads * sizeof (int4), MG_XFER_COPY)) return -1;
  return 0;
}

/* ---- -P ---- */

/* flag[h] = is hit h on a copy-1 mod (modasm.c:926); rd[h] = its read */
__global__ __launch_bounds__ (256)
void mgRsPropFlagKernel (const U32 *__restrict__ hit, U64 nHit, const U64 *__restrict__ hitStart, U32 nReads, const U8 *__restrict__ info, U32 *__restrict__ flag, U32 *__restrict__ rd)
{
  for (U64 h = (U64) blockIdx.x * blockDim.x + threadIdx.x ; h < nHit ; h += (U64) gridDim.x * blockDim.x)
    { flag[h] = (info[hit[h] & MG_TOPMASK] & 3u) == 1u; rd[h] = mgRsReadOf (hitStart, nReads, h); }
}
/* the flagged hits in order: key = the mod, value = the hit's ordinal */
__global__ __launch_bounds__ (256)
void mgRsPropCompactKernel (const U32 *__restrict__ hit, U64 nHit, const U32 *__restrict__ flag, const U32 *__restrict__ place, U32 *__restrict__ key, U32 *__restrict__ val)
{
  for (U64 h = (U64) blockIdx.x * blockDim.x + threadIdx.x ; h < nHit ; h += (U64) gridDim.x * blockDim.x)
    if (flag[h]) { key[place[h]] = hit[h] & MG_TOPMASK; val[place[h]] = (U32) h; }
}
/* sorted[0 .. n): ordinals of the copy-1 hits by mod, in hit order inside a mod, so a run of equal (mod, read) is what one read holds of one mod.
   The lane of a run's first element walks it (runs are short: a mod that a read holds three times is the rare case), counts the forward (bit 31)
   and the reverse hits, classifies as modasm.c:932-941 does and adds to the read's tallies { n, n2Tan, n2Rev, nMoreTan, nMoreRev }; runs of more
   than two are events: evFlag[i] = 1, evCount[i] = f + r, bit 31 of evMod[i] = all in one orientation */
__global__ __launch_bounds__ (256)
void mgRsPropRunKernel (const U32 *__restrict__ sorted, U64 n, const U32 *__restrict__ hit, const U32 *__restrict__ rd, int *__restrict__ tally,
                        U32 *__restrict__ evFlag, U32 *__restrict__ evMod, U32 *__restrict__ evCount)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 o = sorted[i], y = hit[o] & MG_TOPMASK, r = rd[o];
      evFlag[i] = 0;
      if (i) { const U32 q = sorted[i - 1]; if ((hit[q] & MG_TOPMASK) == y && rd[q] == r) continue; }      /* not the first of its run */
      U32 f = 0, rv = 0;
      for (U64 j = i ; j < n ; ++j)
        { const U32 hj = hit[sorted[j]];
          if ((hj & MG_TOPMASK) != y || rd[sorted[j]] != r) break;
          if (hj & ~MG_TOPMASK) ++f; else ++rv;
        }
      int *t = tally + (size_t) r * 5;
      atomicAdd (&t[0], 1);
      if (f + rv == 1) continue;
      if (f == 1 && rv == 1) atomicAdd (&t[2], 1);
      else if (f + rv == 2) atomicAdd (&t[1], 1);
      else
        { const bool tan = !f || !rv;
          atomicAdd (&t[tan ? 3 : 4], 1);
          evFlag[i] = 1; evMod[i] = y | (tan ? ~MG_TOPMASK : 0u); evCount[i] = f + rv;
        }
    }
}
/* the events in order (mod order: the sort's) */
__global__ __launch_bounds__ (256)
void mgRsPropEventKernel (const U32 *__restrict__ sorted, U64 n, const U32 *__restrict__ rd, const U32 *__restrict__ evFlag, const U32 *__restrict__ place,
                          const U32 *__restrict__ evMod, const U32 *__restrict__ evCount, U32 *__restrict__ outRead, U32 *__restrict__ outMod, U32 *__restrict__ outCount)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    if (evFlag[i]) { const U32 e = place[i]; outRead[e] = rd[sorted[i]]; outMod[e] = evMod[i]; outCount[e] = evCount[i]; }
}
/* ev[3 * j ..] = event order[j] as (read, mod | tandem bit, count) */
__global__ __launch_bounds__ (256)
void mgRsPropGatherKernel (const U32 *__restrict__ order, U32 n, const U32 *__restrict__ inRead, const U32 *__restrict__ inMod, const U32 *__restrict__ inCount, U32 *__restrict__ ev)
{
  for (U64 j = (U64) blockIdx.x * blockDim.x + threadIdx.x ; j < n ; j += (U64) gridDim.x * blockDim.x)
    { const U32 e = order[j]; ev[3 * j] = inRead[e]; ev[3 * j + 1] = inMod[e]; ev[3 * j + 2] = inCount[e]; }
}

/* v's hit lists and info[]: in.  hTally[(nReads + 1) * 5]: out, per read { n, n2Tan, n2Rev, nMoreTan, nMoreRev }.  *hEv (malloc ()ed
   here): *nEv triples (read, mod | bit 31 if in one orientation, count), one per mod that a read holds more than twice, by read, by mod inside a read.
   totHit < 2^32 - 16.  0 = done, 1 = the device has no room, -1 = failed */
extern "C" int mgReadsetPropertiesDevice (const MgRsView *v, int *hTally, U32 **hEv, U32 *nEv)
{
  *hEv = 0; *nEv = 0;
  if (mgEnsureDevice ()) return -1;
  const U32 msMax = v->msMax, nReads = v->nReads; const U64 totHit = v->totHit;
  hipStream_t st = 0;
  const size_t m = (size_t) msMax + 1, tallyBytes = ((size_t) nReads + 1) * 5 * sizeof (int);
  const size_t histWords = mgRsSortScratchWords (totHit), scanTiles = mgScanScratchWords (histWords > totHit ? histWords : totHit);
  const size_t bytes = m + ((size_t) nReads + 3) * 8 + tallyBytes + (totHit + 1) * 4 * 9 + scanTiles * 4 + 64;
  if (!mgRsRoom (bytes, totHit)) return 1;
  MgDevScratch scratch ("modasm -P on the device");
  U32 *dHit, *dRd, *dFlag, *dPlace, *dKey, *dVal, *dSorted, *dEvMod, *dEvCount, *dERead, *dEMod, *dECount, *dOrder, *dEv = 0; U64 *dStart; U8 *dInfo; int *dTally;
  if (scratch.get (&dInfo, m) || scratch.get (&dStart, (size_t) nReads + 3) || scratch.get (&dTally, ((size_t) nReads + 1) * 5) || scratch.get (&dHit, totHit + 1)
      || scratch.get (&dRd, totHit + 1) || scratch.get (&dFlag, totHit + 1) || scratch.get (&dPlace, totHit + 1) || scratch.get (&dKey, totHit + 1) || scratch.get (&dVal, totHit + 1)
      || scratch.get (&dEvMod, totHit + 1) || scratch.get (&dEvCount, totHit + 1)) return -1;
  if (hipMemset (dTally, 0, tallyBytes) || hipDeviceSynchronize ()) { scratch.fail (); return -1; }
  if (mgXferH2D (dInfo, v->info, m) || mgXferH2D (dStart, v->hitStart, ((size_t) nReads + 2) * 8) || (totHit && mgXferH2D (dHit, v->hit, totHit * 4))) return -1;
  U32 n1 = 0, nE = 0;                                                /* the copy-1 hits; the events */
  if (totHit)
    { hipLaunchKernelGGL (mgRsPropFlagKernel, dim3 (4096), dim3 (256), 0, st, dHit, totHit, dStart, nReads, dInfo, dFlag, dRd);
      if (mgExclusiveScan (scratch, dFlag, dPlace, totHit, st, &n1)) return -1;
    }
  if (n1)
    { hipLaunchKernelGGL (mgRsPropCompactKernel, dim3 (4096), dim3 (256), 0, st, dHit, totHit, dFlag, dPlace, dKey, dVal);
      if (mgRefStableSort (scratch, dKey, dVal, n1, mgKeyBits (msMax), &dSorted, st)) return -1;
      hipLaunchKernelGGL (mgRsPropRunKernel, dim3 (4096), dim3 (256), 0, st, dSorted, (U64) n1, dHit, dRd, dTally, dFlag, dEvMod, dEvCount);      /* (dFlag, dPlace: free again) */
      if (mgExclusiveScan (scratch, dFlag, dPlace, n1, st, &nE)) return -1;
    }
  if (nE)
    { if (scratch.get (&dERead, nE) || scratch.get (&dEMod, nE) || scratch.get (&dECount, nE) || scratch.get (&dEv, (size_t) nE * 3)) return -1;
      hipLaunchKernelGGL (mgRsPropEventKernel, dim3 (4096), dim3 (256), 0, st, dSorted, (U64) n1, dRd, dFlag, dPlace, dEvMod, dEvCount, dERead, dEMod, dECount);
      if (mgRefStableSort (scratch, dERead, 0, nE, mgKeyBits (nReads), &dOrder, st)) return -1;      /* stable: the events of a read stay in mod order */
      hipLaunchKernelGGL (mgRsPropGatherKernel, dim3 (1024), dim3 (256), 0, st, dOrder, nE, dERead, dEMod, dECount, dEv);
    }
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st)) { scratch.fail (); return -1; }
  U32 *ev = (U32 *) malloc (((size_t) nE ? nE : 1) * 12);
  if (!ev) return -1;
  if (mgXferD2H (hTally, dTally, tallyBytes, MG_XFER_COPY) || (nE && mgXferD2H (ev, dEv, (size_t) nE * 12, MG_XFER_COPY))) { free (ev); return -1; }
  *hEv = ev; *nEv = nE;
  return 0;
}
