/* mg_runtime.hip — what every other file of the library stands on, behind the C ABI of include/modgpu.h: the calling thread's error
 * string, the device check, the alloc / copy / stream wrappers and page-locked memory, the per-kernel event profiler, the hasher's
 * parameters in the form the kernels use, the device pack / unpack / synth wrappers, and mgReleaseBuffers.
 */
#include <stdarg.h>
#include "mg_api_int.h"
#include "mg_xfer.h"

/* ---------------------------------------------------------------------------------------- */
/* errors / device                                                                            */

static thread_local char gErr[512] = "";

void mgSetError (const char *fmt, ...)
{ va_list ap; va_start (ap, fmt); vsnprintf (gErr, sizeof (gErr), fmt, ap); va_end (ap); }

extern "C" const char *mgLastError (void) { return gErr; }

MgStatus mgHipFail (hipError_t e, const char *what)
{ mgSetError ("HIP error %d (%s) in %s", (int) e, hipGetErrorString (e), what); return MG_ERR_HIP; }

extern "C" int mgDeviceCount (void)
{ int n = 0; if (hipGetDeviceCount (&n) != hipSuccess) { (void) hipGetLastError (); return 0; } return n; }

MgStatus mgEnsureDevice (void)
{
  static int known = -1;
  if (known < 0) known = mgDeviceCount ();
  if (known <= 0)
    { mgSetError ("no HIP device available: libmodgpu has no CPU fallback for the batch path");
      return MG_ERR_NO_DEVICE;
    }
  return MG_OK;
}

extern "C" MgStatus mgSetDevice (int device)
{ MgStatus s = mgEnsureDevice (); if (s) return s; MG_HIP (hipSetDevice (device)); return MG_OK; }

extern "C" MgStatus mgDeviceAlloc (void **dptr, size_t bytes)
{ MgStatus s = mgEnsureDevice (); if (s) return s; MG_HIP (hipMalloc (dptr, bytes ? bytes : 16)); return MG_OK; }
extern "C" MgStatus mgDeviceFree (void *dptr) { if (dptr) MG_HIP (hipFree (dptr)); return MG_OK; }
extern "C" MgStatus mgMemcpyH2D (void *dst, const void *src, size_t bytes, void *stream)
{ if (bytes) MG_HIP (hipMemcpyAsync (dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t) stream)); return MG_OK; }
extern "C" MgStatus mgMemcpyD2H (void *dst, const void *src, size_t bytes, void *stream)
{ if (bytes) MG_HIP (hipMemcpyAsync (dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t) stream));
  MG_HIP (hipStreamSynchronize ((hipStream_t) stream)); return MG_OK; }
/* page-locked host memory for the C callers' device-to-host copies (a copy into pageable memory goes through the runtime's staging
   buffers at a few GB/s); portable and mapped: the blocks are kept between calls, and the caller may have moved to another device */
extern "C" void *mgPinnedAlloc (size_t bytes)
{ void *p = 0; if (mgEnsureDevice () || hipHostMalloc (&p, bytes ? bytes : 16, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void) hipGetLastError (); return 0; } return p; }
extern "C" void mgPinnedFree (void *p) { if (p) (void) hipHostFree (p); }
/* device memory to a page-locked block by a kernel that writes host memory, then a wait for the stream: megabytes copied by the
   copy engine take their turn behind a text window (128 MiB) that is on its way to the device at the same time, stores from a kernel
   do not (tools/ubench_copyq.hip) */
__global__ void mgCopyOutKernel (const U64 *__restrict__ src, U64 *__restrict__ dstHost, U64 nWords)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < nWords ; i += (U64) gridDim.x * blockDim.x) dstHost[i] = src[i]; }
extern "C" MgStatus mgCopyOutPinned (void *dstPinned, const void *srcDev, size_t bytes, void *stream)
{
  if (!bytes) return MG_OK;
  void *dDst = 0;
  if ((bytes & 7) || ((uintptr_t) dstPinned & 7) || ((uintptr_t) srcDev & 7) || hipHostGetDevicePointer (&dDst, dstPinned, 0) != hipSuccess)
    { (void) hipGetLastError (); return mgMemcpyD2H (dstPinned, srcDev, bytes, stream); }
  const U64 nWords = bytes >> 3;
  unsigned grid = (unsigned) ((nWords + 255) / 256); if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL (mgCopyOutKernel, dim3 (grid), dim3 (256), 0, (hipStream_t) stream, (const U64 *) srcDev, (U64 *) dDst, nWords);
  MG_HIP (hipGetLastError ());
  MG_HIP (hipStreamSynchronize ((hipStream_t) stream));
  return MG_OK;
}
extern "C" MgStatus mgMemsetD (void *dst, int byte, size_t bytes, void *stream)
{ if (bytes) MG_HIP (hipMemsetAsync (dst, byte, bytes, (hipStream_t) stream)); return MG_OK; }
extern "C" MgStatus mgStreamSynchronize (void *stream)
{ MG_HIP (hipStreamSynchronize ((hipStream_t) stream)); return MG_OK; }

/* ---------------------------------------------------------------------------------------- */
/* per-kernel event timing (bench.py's roofline object)                                       */

static const char *gKernelNames[MG_K_COUNT] = {
  "mgPackKernel", "mgUnpackKernel", "mgTileInfoKernel", "mgScanKernel", "mgTableInsertKernel",
  "mgRankAssignKernel", "mgDirectFlagKernel", "mgTableFindKernel", "mgTableLoadKernel",
  "mgTableExportDepthKernel", "mgTableHistKernel", "mgReplayIndexKernel", "mgIndexFinishKernel",
  "mgSynthGenomeKernel", "mgSynthReadsKernel", "memset", "mgSegScanKernel", "mgSegCompactKernel",
  "mgPartChunks+ScanKernel", "mgPartHistKernel", "mgPartScatterKernel", "mgRankCountKernel", "mgRankScanKernel", "mgBucketDedupKernel",
  "mgBucketMergeKernel", "mgRankLookupKernel", "mgTableFindSegKernel", "mgHotPlan+ReduceKernel", "mgBucketFindKernel", "mgUnpartKernel", "mgChainKernel", "mgChainResolveKernel",
  "mgPaintItemsKernel", "mgDepthGuardKernel", "mgDepthGatherKernel", "mgTextLenKernel", "mgTextScanKernel", "mgTextWriteKernel",
  "mgSetTextLinesKernel", "mgSetTextScanKernel", "mgSetTextParseKernel", "mgSetTextLastKernel",
  "mgOvElem..TableKernels", "mgOvEmitKernel", "overlap sorts", "mgOvHead..PairInitKernels", "mgOvPairKernel",
  "mgTrimSkip+OffsetsKernel", "mgTrimGatherKernel", "mgSetCopyKernel", "mgCopyTallyKernel", "mgRankRecordKernel" };
#define MG_PROF_POOL 8192
struct MgProfRec { int id; hipEvent_t a, b; };
static struct {
  bool on = false;
  int only = -1;                 /* >= 0: bracket launches of this kernel id alone */
  MgProfRec rec[MG_PROF_POOL]; int used = 0, made = 0;
  double ms[MG_K_COUNT] = { 0 }; U64 n[MG_K_COUNT] = { 0 };
  int open = -1;
} gProf;

static void mgProfDrain (void)
{
  if (!gProf.used) return;
  (void) hipDeviceSynchronize ();
  for (int i = 0 ; i < gProf.used ; ++i)
    { float t = 0;
      if (hipEventElapsedTime (&t, gProf.rec[i].a, gProf.rec[i].b) == hipSuccess)
        { gProf.ms[gProf.rec[i].id] += t; ++gProf.n[gProf.rec[i].id]; }
    }
  gProf.used = 0;
}

void mgProfBegin (int id, hipStream_t st)
{
  if (!gProf.on || (gProf.only >= 0 && id != gProf.only)) return;
  if (gProf.used == MG_PROF_POOL) mgProfDrain ();
  MgProfRec &r = gProf.rec[gProf.used];
  if (gProf.used >= gProf.made)
    { if (hipEventCreate (&r.a) != hipSuccess || hipEventCreate (&r.b) != hipSuccess) { gProf.on = false; return; }
      gProf.made = gProf.used + 1;
    }
  r.id = id;
  (void) hipEventRecord (r.a, st);
  gProf.open = gProf.used;
}

void mgProfEnd (int id, hipStream_t st)
{
  if (!gProf.on || gProf.open < 0) return;
  (void) id;
  (void) hipEventRecord (gProf.rec[gProf.open].b, st);
  gProf.used = gProf.open + 1;
  gProf.open = -1;
}

extern "C" void mgProfileEnable (int on) { if (!on) mgProfDrain (); gProf.on = on != 0; }
extern "C" void mgProfileOnly (int kernelId) { mgProfDrain (); gProf.only = (kernelId >= 0 && kernelId < MG_K_COUNT) ? kernelId : -1; }
extern "C" void mgProfileReset (void)
{ mgProfDrain (); for (int i = 0 ; i < MG_K_COUNT ; ++i) { gProf.ms[i] = 0; gProf.n[i] = 0; } }
extern "C" int mgProfileKernels (void) { return MG_K_COUNT; }
extern "C" MgStatus mgProfileGet (int id, const char **name, double *totalMs, U64 *launches)
{
  if (id < 0 || id >= MG_K_COUNT) { mgSetError ("bad kernel id"); return MG_ERR_ARG; }
  mgProfDrain ();
  if (name) *name = gKernelNames[id];
  if (totalMs) *totalMs = gProf.ms[id];
  if (launches) *launches = gProf.n[id];
  return MG_OK;
}

/* ---------------------------------------------------------------------------------------- */
/* hash parameters                                                                            */

MgHashParams mgMakeParams (const Seqhash *sh)
{
  MgHashParams p;
  p.factor1 = sh->factor1; p.mask = sh->mask; p.k = sh->k; p.shift1 = sh->shift1;
  p.d = (U32) sh->w;
  p.dShift = __builtin_ctz (p.d);
  U64 odd = (U64) (p.d >> p.dShift);
  U64 x = odd;                                   /* Newton: inverse of an odd number mod 2^64 */
  for (int i = 0 ; i < 6 ; ++i) x *= 2 - odd * x;
  p.dOddInv = x;
  p.dOddLim = ~(U64) 0 / odd;
  p.small32 = (2 * sh->k <= 40 && odd < ((U64) 1 << 15)) ? 1u : 0u;
  p.c24 = (U32) (((U64) 1 << 24) % odd); p.inv32 = (U32) x; p.lim32 = (U32) (0xffffffffull / odd);
  return p;
}

MgStatus mgCheckHasher (const Seqhash *sh)
{
  if (!sh || sh->k < 1 || sh->k >= 32 || sh->w < 1 || sh->shift1 != 64 - 2 * sh->k)
    { mgSetError ("invalid Seqhash (k %d w %d)", sh ? sh->k : -1, sh ? sh->w : -1); return MG_ERR_ARG; }
  return MG_OK;
}

/* ---------------------------------------------------------------------------------------- */
/* packing and synthetic data on the device (mgPackHost, mgPackWords: mg_pack.c)              */

extern "C" size_t mgPackedWords (U64 nBases) { return (size_t) ((nBases + 15) / 16) + MG_PACK_PAD; }

extern "C" MgStatus mgPackDevice (const U8 *dBases, U64 nBases, U32 *dWords, void *stream)
{ MgStatus s = mgEnsureDevice (); if (s) return s; return mgLaunchPack (dBases, nBases, dWords, (hipStream_t) stream); }
extern "C" MgStatus mgUnpackDevice (const U32 *dWords, U64 nBases, U8 *dBases, void *stream)
{ MgStatus s = mgEnsureDevice (); if (s) return s; return mgLaunchUnpack (dWords, nBases, dBases, (hipStream_t) stream); }

extern "C" MgStatus mgSynthGenome (U32 *dPacked, U64 nBases, U64 seed, void *stream)
{ MgStatus s = mgEnsureDevice (); if (s) return s; return mgLaunchSynthGenome (dPacked, nBases, seed, (hipStream_t) stream); }

extern "C" MgStatus mgSynthReads (const U32 *dGenomePacked, U64 genomeBases,
                                  const U64 *dReadStart, const U64 *dReadOffsets, const U8 *dStrand, U32 nReads,
                                  U64 totalBases, double errRate, U64 seed, U32 *dPackedOut, void *stream)
{ MgStatus s = mgEnsureDevice (); if (s) return s;
  return mgLaunchSynthReads (dGenomePacked, genomeBases, dReadStart, dReadOffsets, dStrand, nReads, totalBases,
                             errRate, seed, dPackedOut, (hipStream_t) stream);
}

extern "C" void mgReleaseBuffers (void)      /* everything the library caches between calls */
{
  mgSeqReleaseBuffers ();
  mgTextReleaseBuffers ();
  mgQueryReleaseBuffers ();
  mgHostBatchRelease ();
  mgIterReleaseBuffers ();
  mgXferReleaseBuffers ();
  mgUploadRelease ();
}
