/* mg_refpack.hip — modmap's Reference built on the device: the bookkeeping of referenceFastaRead
 * (modmap.c:106-118: per occurrence index / offset / id, ++depth[index]), the copy classes (modmap.c:125-129) and
 * referencePack (modmap.c:74-91: loc = exclusive sums of depth, rev = the occurrences grouped by modset index, in
 * occurrence order inside an index).
 *
 * The seeds of a batch -- (index, pos, sequence) per modimizer, in (sequence, pos) order -- are dense on the device when
 * mgInsertReadsDevice / mgQueryReadsDevice return.  They stay there:
 *   append    ordered compaction of the seeds with index != 0 (modmap.c:110) behind what the reference holds already,
 *             pos masked, id = first id of the batch + sequence ordinal, depth counted with atomics (a count: order free);
 *   finish    info[] classified from depth (one pass, the three tallies reduced per workgroup); loc[] by the device-wide
 *             exclusive scan and rev[] by the STABLE radix sort of mg_devsort.hip, of (index, occurrence ordinal): stability is
 *             what keeps the occurrences of one index in occurrence order, which modmap.c:86-90 produces by walking the
 *             occurrences in order and queryProcess relies on (rev[loc[x]] is the FIRST occurrence, rev[loc[x] + 1] the second:
 *             modmap.c:219-221,242-254);
 *   mirror    the six arrays go back to the host's Reference in one piece each (mg_xfer.hip); what stays resident is what
 *             mg_chain.hip's chaining reads, derived from them: li[x] = loc[x] | info[x] << 32 and revid[j] = rev[j] | id[rev[j]] << 32
 *             (one 8-byte load gives a seed its copy class and CSR offset, one or two adjacent ones its first two occurrences with
 *             the sequences they lie on) and offset[] -- no re-upload.
 * A Reference whose arrays came from a file (mgReferenceLoad) or were written by the host is uploaded and the same words derived.
 * The arrays of MgRefDev live as long as the Reference does; what a call needs besides them is its MgDevScratch's.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <mutex>
#include <unordered_map>
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_xfer.h"
#include "mg_ref.h"
#include "mg_devsort.h"

/* the device side of every Reference, by its address.  The lock guards the MAP (finding, making and dropping an entry); an entry itself belongs
   to the Reference, which -- like the reference's own struct -- one host thread works on at a time: builds of two References on two GPUs run
   side by side.  (An unordered_map keeps its elements where they are when it grows: the entry found under the lock stays valid after it.) */
static std::mutex gRefLock;
static std::unordered_map<const MgReference *, MgRefDev> gRefDev;
static std::unordered_map<const MgReference *, std::mutex> gRefOwn;      /* one lock per Reference: two threads that query ONE Reference do not both build its device side */
static MgRefDev &mgRefEntry (const MgReference *ref) { std::lock_guard<std::mutex> g (gRefLock); return gRefDev[ref]; }
static std::mutex &mgRefOwnLock (const MgReference *ref) { std::lock_guard<std::mutex> g (gRefLock); return gRefOwn[ref]; }

static void mgRefDevFree (MgRefDev &d)
{ (void) hipFree (d.info); (void) hipFree (d.loc); (void) hipFree (d.rev); (void) hipFree (d.id); (void) hipFree (d.offset);
  (void) hipFree (d.index); (void) hipFree (d.depth); (void) hipFree (d.li); (void) hipFree (d.revid); d = MgRefDev ();
}

/* li[] and revid[] (mg_ref.h) from info / loc / rev / id; those four are freed: the chaining reads the derived words only */
__global__ void mgRefDeriveLiKernel (const U8 *__restrict__ info, const U32 *__restrict__ loc, U64 m, U64 *__restrict__ li)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < m ; i += (U64) gridDim.x * blockDim.x) li[i] = (U64) loc[i] | ((U64) info[i] << 32); }
__global__ void mgRefDeriveRevidKernel (const U32 *__restrict__ rev, const U32 *__restrict__ id, U64 n, U64 *__restrict__ revid)      /* n = ref->max; slot n: occurrence 0 */
{ for (U64 j = (U64) blockIdx.x * blockDim.x + threadIdx.x ; j <= n ; j += (U64) gridDim.x * blockDim.x) { const U32 r = j < n ? rev[j] : 0u; revid[j] = (U64) r | ((U64) (n ? id[r] : 0u) << 32); } }
static MgStatus mgRefDerive (MgRefDev &d, U32 msMax, U32 refMax, hipStream_t st)
{
  const U64 m = (U64) msMax + 1, n = refMax;
  if (d.nSeq >= (1 << 29)) { mgSetError ("more than 2^29 reference sequences"); return MG_ERR_ARG; }      /* (the chaining's seed records keep three flag bits above the sequence id) */
  (void) hipFree (d.li); d.li = 0; (void) hipFree (d.revid); d.revid = 0;
  MG_HIP (hipMalloc ((void **) &d.li, m * 8));
  MG_HIP (hipMalloc ((void **) &d.revid, (n + 1) * 8));
  hipLaunchKernelGGL (mgRefDeriveLiKernel, dim3 (2048), dim3 (256), 0, st, d.info, d.loc, m, d.li);
  hipLaunchKernelGGL (mgRefDeriveRevidKernel, dim3 (2048), dim3 (256), 0, st, d.rev, d.id, n, d.revid);
  MG_HIP (hipGetLastError ());
  MG_HIP (hipStreamSynchronize (st));
  (void) hipFree (d.info); d.info = 0; (void) hipFree (d.loc); d.loc = 0; (void) hipFree (d.rev); d.rev = 0; (void) hipFree (d.id); d.id = 0;
  return MG_OK;
}

extern "C" void mgChainForget (const MgReference *ref)
{
  std::lock_guard<std::mutex> g (gRefLock);
  auto it = gRefDev.find (ref);
  if (it != gRefDev.end ()) { mgRefDevFree (it->second); gRefDev.erase (it); }
  gRefOwn.erase (ref);                                 /* (the Reference is going: nobody holds its lock) */
}

/* device copies of what the chaining reads: the ones the builder left, or uploaded from the host arrays (a Reference read from a
   file, or one whose modset has grown since) */
MgStatus mgRefDevGet (const MgReference *ref, MgRefDev *out)
{
  std::lock_guard<std::mutex> own (mgRefOwnLock (ref));
  MgRefDev &d = mgRefEntry (ref);
  const U32 msMax = ref->ms->max, refMax = ref->max;
  int cur = 0; MG_HIP (hipGetDevice (&cur));
  if (d.li && d.packed && d.msMax == msMax && d.refMax == refMax && d.device == cur) { *out = d; return MG_OK; }
  mgRefDevFree (d);                                    /* (also: made on another GPU than the one the calling thread is on now -- uploaded again, here) */
  d.device = cur;
  const size_t m = (size_t) msMax + 1, n = refMax ? refMax : 1;
  MG_HIP (hipMalloc ((void **) &d.info, m));
  MG_HIP (hipMalloc ((void **) &d.loc, m * 4));
  MG_HIP (hipMalloc ((void **) &d.rev, (n + 1) * 4));
  MG_HIP (hipMalloc ((void **) &d.id, n * 4));
  MG_HIP (hipMalloc ((void **) &d.offset, n * 4));
  MG_HIP (hipMemset (d.rev, 0, (n + 1) * 4));
  MG_HIP (hipDeviceSynchronize ());
  MgStatus s;
  if ((s = mgXferH2D (d.info, ref->ms->info, m)) || (s = mgXferH2D (d.loc, ref->loc, m * 4))) return s;
  if (refMax && ((s = mgXferH2D (d.rev, ref->rev, (size_t) refMax * 4)) || (s = mgXferH2D (d.id, ref->id, (size_t) refMax * 4))
                 || (s = mgXferH2D (d.offset, ref->offset, (size_t) refMax * 4)))) return s;
  d.nSeq = ref->nSeq;
  if ((s = mgRefDerive (d, msMax, refMax, 0))) return s;
  d.msMax = msMax; d.refMax = refMax; d.packed = true;
  *out = d;
  return MG_OK;
}

/* ---------------------------------------------------------------------------------------- */
/* append: modmap.c:110-117 for a batch of seeds                                              */

__global__ __launch_bounds__ (256)
void mgRefCountHitsKernel (const U32 *__restrict__ ix, U64 n, U32 *__restrict__ tileCount)
{
  __shared__ U32 lds[4];
  const U64 base = (U64) blockIdx.x * MG_SCAN_TILE;
  U32 s = 0;
  for (int j = 0 ; j < 16 ; ++j) { const U64 i = base + (U64) j * 256 + threadIdx.x; if (i < n && ix[i]) ++s; }
  s = mgBlockReduce<256, MgSum> (s, lds);
  if (!threadIdx.x) tileCount[blockIdx.x] = s;
}
/* tile b's hits go to at0 + tileBase[b] .. in order: inside the tile a wave takes 64 consecutive seeds at a time (ballot + popcount),
   the four waves one after the other over the tile's 16 rows of 256 */
__global__ __launch_bounds__ (256)
void mgRefAppendKernel (const U32 *__restrict__ ix, const U32 *__restrict__ posF, const U32 *__restrict__ rid, U64 n, const U32 *__restrict__ tileBase,
                        U32 at0, U32 idBase, U32 *__restrict__ index, U32 *__restrict__ offset, U32 *__restrict__ id, U32 *__restrict__ depth)
{
  __shared__ U32 sRow[64];                                         /* hits per (row of 256, wave): 16 x 4 */
  const U64 base = (U64) blockIdx.x * MG_SCAN_TILE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  U32 x[16];
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j)
    { const U64 i = base + (U64) j * 256 + threadIdx.x;
      x[j] = i < n ? ix[i] : 0u;
      const U64 b = __ballot (x[j] != 0);
      if (!lane) sRow[j * 4 + w] = (U32) __popcll (b);
    }
  __syncthreads ();
  if (threadIdx.x == 0) { U32 run = 0; for (int q = 0 ; q < 64 ; ++q) { const U32 c = sRow[q]; sRow[q] = run; run += c; } }
  __syncthreads ();
  const U32 tb = at0 + tileBase[blockIdx.x];
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j)
    { const U64 i = base + (U64) j * 256 + threadIdx.x;
      const U64 b = __ballot (x[j] != 0);
      if (x[j])
        { const U32 at = tb + sRow[j * 4 + w] + (U32) __popcll (b & (((U64) 1 << lane) - 1));
          index[at] = x[j]; offset[at] = posF[i] & MG_POS_MASK; id[at] = idBase + rid[i];
          atomicAdd (&depth[x[j]], 1u);
        }
    }
}

/* ---------------------------------------------------------------------------------------- */
/* finish: copy classes, loc, rev                                                             */

/* modmap.c:125-129: depth 1 -> copy 1, 2 -> copy 2, anything else (0 included) -> copy M; entries 1 .. max; tallies[3] */
__global__ __launch_bounds__ (256)
void mgRefClassifyKernel (const U32 *__restrict__ depth, U32 max, U8 *__restrict__ info, U32 *__restrict__ tallies)
{
  __shared__ U32 sT[3];
  if (threadIdx.x < 3) sT[threadIdx.x] = 0;
  __syncthreads ();
  U32 c1 = 0, c2 = 0, cM = 0;
  for (U64 i = 1 + (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= max ; i += (U64) gridDim.x * blockDim.x)
    { const U32 dp = depth[i]; const U8 f = info[i];
      if (dp == 1) { info[i] = (U8) ((f & 0xfc) | 1); ++c1; }
      else if (dp == 2) { info[i] = (U8) ((f & 0xfc) | 2); ++c2; }
      else { info[i] = (U8) (f | 3); ++cM; }
    }
  c1 = mgWaveReduce<MgSum> (c1); c2 = mgWaveReduce<MgSum> (c2); cM = mgWaveReduce<MgSum> (cM);
  if ((threadIdx.x & 63) == 0) { atomicAdd (&sT[0], c1); atomicAdd (&sT[1], c2); atomicAdd (&sT[2], cM); }
  __syncthreads ();
  if (threadIdx.x < 3 && sT[threadIdx.x]) atomicAdd (&tallies[threadIdx.x], sT[threadIdx.x]);
}

/* ---------------------------------------------------------------------------------------- */

static MgStatus mgRefGrow (U32 **p, size_t have, size_t keep, size_t want)      /* device array of `want` words holding the first `keep` of the old one */
{
  (void) have;
  U32 *q = 0;
  MG_HIP (hipMalloc ((void **) &q, (want ? want : 1) * 4));
  if (*p && keep) MG_HIP (hipMemcpy (q, *p, keep * 4, hipMemcpyDeviceToDevice));
  if (*p) MG_HIP (hipFree (*p));
  *p = q;
  return MG_OK;
}

/* a Reference is built on the GPU its first batch came to: the arrays of d are that one's */
static MgStatus mgRefBuildOnThisDevice (MgRefDev &d)
{
  int cur = 0; MG_HIP (hipGetDevice (&cur));
  if (d.device >= 0 && d.device != cur && d.depth) { mgSetError ("this Reference is being built on GPU %d, the calling thread is on GPU %d", d.device, cur); return MG_ERR_ARG; }
  d.device = cur;
  return MG_OK;
}

/* *cnt = how many of the n seeds have an index; *tiles (the scratch's): per tile of MG_SCAN_TILE seeds the hits before it, what mgRefAppendKernel places by */
static MgStatus mgRefCountHits (MgDevScratch &scratch, const U32 *dIx, U64 n, hipStream_t st, U32 **tiles, U32 *cnt)
{
  const U32 nTiles = (U32) ((n + MG_SCAN_TILE - 1) / MG_SCAN_TILE);
  if (scratch.get (tiles, (size_t) nTiles + 2)) return MG_ERR_HIP;
  hipLaunchKernelGGL (mgRefCountHitsKernel, dim3 (nTiles), dim3 (256), 0, st, dIx, n, *tiles);
  hipLaunchKernelGGL ((mgGroupSumKernel<U32, U32>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, *tiles, *tiles, nTiles, *tiles + nTiles);
  if (hipMemcpyAsync (cnt, *tiles + nTiles, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess) return scratch.fail ();
  return MG_OK;
}

/* the seeds of a batch (device arrays, n of them, in order) behind the ref->max occurrences held so far; *appended = how many had an index */
extern "C" MgStatus mgRefBuildAppend (MgReference *ref, const U32 *dIx, const U32 *dPosF, const U32 *dRid, U64 n, U32 idBase, U32 *appended)
{
  *appended = 0;
  std::lock_guard<std::mutex> own (mgRefOwnLock (ref));
  MgRefDev &d = mgRefEntry (ref);
  hipStream_t st = 0;
  MgDevScratch scratch ("reference append");
  MgStatus s;
  U32 *tiles, cnt = 0;
  if (d.packed)
    { /* a further file read into a packed Reference: referencePack left size == max (modmap.c:80), so the reference dies on the FIRST seed
         that has an index (modmap.c:111) and otherwise goes on, adds nothing and reports again */
      if (!n) return MG_OK;
      if ((s = mgRefCountHits (scratch, dIx, n, st, &tiles, &cnt))) return s;
      if (cnt) { mgSetError ("reference size overflow"); return MG_ERR_CAPACITY; }
      return MG_OK;
    }
  if ((s = mgRefBuildOnThisDevice (d))) return s;
  const size_t msCap = ref->ms->size;
  if (!d.depth)
    { MG_HIP (hipMalloc ((void **) &d.depth, (msCap + 1) * 4));
      MG_HIP (hipMemsetAsync (d.depth, 0, (msCap + 1) * 4, st));
      d.capMs = msCap;
      if (ref->max)                                                  /* occurrences the host holds already (a caller that filled the arrays itself) */
        { mgSetError ("mgRefBuildAppend: a reference with host-built occurrences cannot be extended on the device"); return MG_ERR_ARG; }
    }
  if (!n) return MG_OK;
  if (n >= ((U64) 1 << 32)) { mgSetError ("too many seeds in one batch"); return MG_ERR_ARG; }
  if ((s = mgRefCountHits (scratch, dIx, n, st, &tiles, &cnt))) return s;
  /* modmap.c:111: an append is refused once max + 1 >= size */
  if (cnt && (U64) ref->max + cnt > (U64) ref->size - 1) { mgSetError ("reference size overflow"); return MG_ERR_CAPACITY; }
  const size_t want = (size_t) ref->max + cnt;
  if (want > d.capOcc)
    { size_t cap = want + want / 2 + 65536; if (cap > ref->size) cap = ref->size; if (cap < want) cap = want;
      if ((s = mgRefGrow (&d.index, d.capOcc, ref->max, cap)) || (s = mgRefGrow (&d.offset, d.capOcc, ref->max, cap)) || (s = mgRefGrow (&d.id, d.capOcc, ref->max, cap))) return s;
      d.capOcc = cap;
    }
  if (cnt)
    { const U32 nTiles = (U32) ((n + MG_SCAN_TILE - 1) / MG_SCAN_TILE);
      hipLaunchKernelGGL (mgRefAppendKernel, dim3 (nTiles), dim3 (256), 0, st, dIx, dPosF, dRid, n, tiles, ref->max, idBase, d.index, d.offset, d.id, d.depth);
      if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st) != hipSuccess) return scratch.fail ();
    }
  *appended = cnt;
  return MG_OK;
}

/* 1 (and the tallies of its copy classes) if ref is packed on the device and nothing came since: what a further mgReferenceFinish reports again */
extern "C" int mgRefPackedTallies (MgReference *ref, U32 tallies[3])
{
  std::lock_guard<std::mutex> own (mgRefOwnLock (ref));
  MgRefDev &d = mgRefEntry (ref);
  if (!d.packed || d.refMax != ref->max || d.msMax != ref->ms->max) return 0;
  tallies[0] = d.tallies[0]; tallies[1] = d.tallies[1]; tallies[2] = d.tallies[2];
  return 1;
}

/* modmap.c:125-129 + 74-91.  The host arrays are the caller's, sized as referencePack sizes them: index / offset / id / rev
   [ref->max], depth / loc [ms->max + 1], info = ms->info; tallies[3] = copy 1, copy 2, multiple. */
extern "C" MgStatus mgRefBuildFinish (MgReference *ref, U32 *hIndex, U32 *hOffset, U32 *hId, U32 *hDepth, U32 *hRev, U32 *hLoc, U8 *hInfo, U32 tallies[3])
{
  std::lock_guard<std::mutex> own (mgRefOwnLock (ref));
  MgRefDev &d = mgRefEntry (ref);
  hipStream_t st = 0;
  const U32 msMax = ref->ms->max, n = ref->max;
  const size_t m = (size_t) msMax + 1;
  tallies[0] = tallies[1] = tallies[2] = 0;
  struct timespec tq0; clock_gettime (CLOCK_MONOTONIC, &tq0);
  const bool lapOn = mgKnobs ()->seedTiming == 1;
#define MG_LAP(what) do { if (lapOn) { (void) hipStreamSynchronize (st); struct timespec q_; clock_gettime (CLOCK_MONOTONIC, &q_); fprintf (stderr, "mgRefBuildFinish: %s at %.1f ms\n", what, (q_.tv_sec - tq0.tv_sec) * 1e3 + (q_.tv_nsec - tq0.tv_nsec) * 1e-6); } } while (0)
  if (d.packed) { mgSetError ("the reference is packed already"); return MG_ERR_ARG; }
  MgStatus s;
  if ((s = mgRefBuildOnThisDevice (d))) return s;
  if (!d.depth)                                                      /* no batch ever came: an empty reference */
    { MG_HIP (hipMalloc ((void **) &d.depth, (m + 1) * 4)); MG_HIP (hipMemsetAsync (d.depth, 0, (m + 1) * 4, st)); d.capMs = m; }
  if (m > d.capMs + 1) { mgSetError ("modset grew beyond its size"); return MG_ERR_CAPACITY; }
  MgDevScratch scratch ("reference pack on the device");
  U32 *dTal;
  if (scratch.get (&dTal, 4)) return MG_ERR_HIP;
  if (hipMemsetAsync (dTal, 0, 16, st)) return scratch.fail ();
  /* info: the host's flag bytes up, the copy classes set, back down (and kept for the chaining) */
  (void) hipFree (d.info); d.info = 0; (void) hipFree (d.loc); d.loc = 0;
  if (hipMalloc ((void **) &d.info, m) || hipMalloc ((void **) &d.loc, (m + 1) * 4) || hipStreamSynchronize (st)) return scratch.fail ();
  MG_LAP ("allocations");
  if ((s = mgXferH2DSparse (d.info, hInfo, m))) return s;
  MG_LAP ("info up");      /* (a new Modset's info[] has never been written: nothing is read, and the mirror below lands on fresh pages) */
  if (msMax) hipLaunchKernelGGL (mgRefClassifyKernel, dim3 (2048), dim3 (256), 0, st, d.depth, msMax, d.info, dTal);
  if ((s = mgExclusiveScan (scratch, d.depth, d.loc, m, st))) return s;
  MG_LAP ("classes + loc");
  if (hipMemcpyAsync (tallies, dTal, 12, hipMemcpyDeviceToHost, st)) return scratch.fail ();
  /* rev: the occurrence ordinals sorted by index, stably */
  (void) hipFree (d.rev); d.rev = 0;
  if (n)
    { MG_LAP ("sort allocations");
      U32 *rev;
      if ((s = mgRefStableSort (scratch, d.index, 0, n, mgKeyBits (msMax), &rev, st))) return s;
      d.rev = scratch.take (rev);
      MG_LAP ("sort");
      if (hipMemsetAsync (d.rev + n, 0, 4, st)) return scratch.fail ();      /* (the chaining reads rev[loc[x] + 1] of a copy-2 seed: inside the array, but keep the slack defined) */
    }
  else { if (hipMalloc ((void **) &d.rev, 8) || hipMemsetAsync (d.rev, 0, 8, st)) return scratch.fail (); }
  if (hipStreamSynchronize (st)) return scratch.fail ();
  MG_LAP ("kernels done");
  /* mirror */
  if ((s = mgXferD2H (hInfo, d.info, m, MG_XFER_COPY)) || (s = mgXferD2H (hDepth, d.depth, m * 4, MG_XFER_COPY)) || (s = mgXferD2H (hLoc, d.loc, m * 4, MG_XFER_COPY))) return s;
  if (n && ((s = mgXferD2H (hIndex, d.index, (size_t) n * 4, MG_XFER_COPY)) || (s = mgXferD2H (hOffset, d.offset, (size_t) n * 4, MG_XFER_COPY))
            || (s = mgXferD2H (hId, d.id, (size_t) n * 4, MG_XFER_COPY)) || (s = mgXferD2H (hRev, d.rev, (size_t) n * 4, MG_XFER_COPY)))) return s;
  /* what the chaining does not read goes; the rest is the resident copy */
  (void) hipFree (d.index); d.index = 0; (void) hipFree (d.depth); d.depth = 0; d.capOcc = 0; d.capMs = 0;
  if (!d.id) { if (hipMalloc ((void **) &d.id, 8) || hipMalloc ((void **) &d.offset, 8) || hipMemset (d.id, 0, 8)) return scratch.fail (); }
  d.nSeq = ref->nSeq;
  MG_LAP ("mirror");
  if ((s = mgRefDerive (d, msMax, n, st))) return s;
  MG_LAP ("derive");
  d.msMax = msMax; d.refMax = n; d.packed = true;
  d.tallies[0] = tallies[0]; d.tallies[1] = tallies[1]; d.tallies[2] = tallies[2];
  return MG_OK;
}
