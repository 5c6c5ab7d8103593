/* mg_inflate.hip — gzip members of at most 64 KiB (BGZF: bgzip, htslib) inflated on the device: the kernel, mgInflateMembersDevice and
 * the host compile of the decoder (mgInflateMemberHost).  The decoder itself is mg_inflate_core.h, written once for both sides.
 *
 * Shape: one wave a member, one wave a workgroup, workgroup m of the launch takes member m of the table.
 *   - Symbol decode is serial within a member: LANE 0 runs mgInfInflate -- code tables, symbols, literals and matches.  The other lanes
 *     fill the CRC table while it starts and take their slices of the CRC when it is done; until then they wait at the barrier.  (The
 *     tables are rebuilt per deflate block by the decoding lane as well: a few hundred entries against thousands of symbols.)
 *   - LDS: one MgInfTables, 4608 bytes, per wave (sizes at its declaration).  160 KiB a CU hold 35; a CU runs at most 32 waves, so LDS
 *     does not bound how many members a CU decodes at once.
 *   - Back-references go through global memory: the member's output, up to 64 KiB, has no room in LDS beside the tables.  A match is
 *     read and written by the SAME lane (lane 0, byte by byte in program order), so that is no cross-lane hand-off and needs no fence:
 *     a thread's loads see its own earlier stores.
 *   - The CRC is the one cross-lane hand-off through memory: lane 0 has stored the text, all 64 lanes load it.  __syncthreads () stands
 *     between the two -- a workgroup-scope release, the barrier and a workgroup-scope acquire (the workgroup is this one wave, so this is
 *     wavefront-scope ordering and more) -- it also publishes the CRC table in LDS.  Each lane takes a contiguous slice, the slices' CRCs
 *     are shifted to their place by the CRC's linearity (zlib's crc32_combine arithmetic, mg_inflate_core.h) and xor-ed across the wave.
 *   - Per-member status: a bad member sets its own word and the launch's counter, the others are not touched.  Nothing is written past
 *     uOff + uLen: the decoder tests every literal and every match against the stated length first. */
#include <string.h>
#include "mg_common.h"
#include "mg_internal.h"
#include "mg_inflate_core.h"

#define INF_THREADS 64
#define INF_MAX 65536u                                   /* bytes of a member, compressed or not */

__global__ __launch_bounds__ (INF_THREADS)
void mgInflateKernel (const U8 *__restrict__ comp, const MgGzMember *__restrict__ members, U32 n, U8 *out, int checkCrc, U32 *__restrict__ status, U32 *__restrict__ nBad)
{
  __shared__ MgInfTables T;
  const U32 m = blockIdx.x, lane = threadIdx.x;
  if (m >= n) return;
  const MgGzMember g = members[m];
  U8 *text = out + g.uOff;
  mgInfCrcTable (T.crcTab, lane, INF_THREADS);
  U32 st = 0;
  if (lane == 0) st = mgInfInflate (comp + g.cOff, g.cLen, text, g.uLen, &T, 0);
  __syncthreads ();                                      /* lane 0's text, every lane's table entries: visible to the wave from here */
  st = (U32) __shfl ((int) st, 0);
  if (!st && checkCrc)
    { U32 c = mgInfCrcSlice (T.crcTab, text, g.uLen, lane);
      for (int d = 32 ; d ; d >>= 1) c ^= (U32) __shfl_xor ((int) c, d);
      if (c != g.crc) st = MGI_CRC;
    }
  if (lane == 0)
    { status[m] = st;
      if (st) atomicAdd (nBad, 1u);
    }
}

static thread_local U64 gInfDiag[4];                     /* members inflated on the device, compressed bytes uploaded, text bytes produced, kernel launches */
extern "C" void mgInflateDiag (U64 out4[4]) { memcpy (out4, gInfDiag, sizeof (gInfDiag)); }
extern "C" void mgInflateDiagReset (void) { memset (gInfDiag, 0, sizeof (gInfDiag)); }
extern "C" void mgInflateDiagUploaded (U64 bytes) { gInfDiag[1] += bytes; }

static int infCheck (const MgGzMember *members, U32 n, U64 compBytes, U64 outBytes)
{
  for (U32 i = 0 ; i < n ; ++i)
    { const MgGzMember &g = members[i];
      if (g.cLen > INF_MAX || g.uLen > INF_MAX)
        { mgSetError ("mgInflateMembersDevice: member %u of %u compressed and %u inflated bytes: at most %u either way", i, g.cLen, g.uLen, INF_MAX); return -1; }
      if (g.cOff > compBytes || g.cLen > compBytes - g.cOff || g.uOff > outBytes || g.uLen > outBytes - g.uOff)
        { mgSetError ("mgInflateMembersDevice: member %u leaves its buffer", i); return -1; }
    }
  return 0;
}

/* the launch for a caller that owns the device arrays (mg_bgzfsrc.hip): dWork holds n members, then n + 1 words (statuses, the counter) */
extern "C" MgStatus mgInflateRun (const U8 *dComp, U64 compBytes, const MgGzMember *members, U32 n, U8 *dOut, U64 outBytes, void *dWork, U32 *status, U32 *nBad, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  if (nBad) *nBad = 0;
  if (!n) return MG_OK;
  if (!members || !dComp || !dOut) { mgSetError ("mgInflateMembersDevice: null argument"); return MG_ERR_ARG; }
  if (infCheck (members, n, compBytes, outBytes)) return MG_ERR_ARG;
  MgGzMember *dMem = (MgGzMember *) dWork;
  U32 *dStatus = (U32 *) (dMem + n);
  U32 bad = 0; U64 text = 0;
  for (U32 i = 0 ; i < n ; ++i) text += members[i].uLen;
  MG_HIP (hipMemcpyAsync (dMem, members, (size_t) n * sizeof (MgGzMember), hipMemcpyHostToDevice, st));
  MG_HIP (hipMemsetAsync (dStatus + n, 0, 4, st));
  hipLaunchKernelGGL (mgInflateKernel, dim3 (n), dim3 (INF_THREADS), 0, st, dComp, dMem, n, dOut, mgKnobs ()->inflateNoCrc == 1 ? 0 : 1, dStatus, dStatus + n);
  MG_HIP (hipGetLastError ());
  MG_HIP (hipMemcpyAsync (&bad, dStatus + n, 4, hipMemcpyDeviceToHost, st));
  if (status) MG_HIP (hipMemcpyAsync (status, dStatus, (size_t) n * 4, hipMemcpyDeviceToHost, st));
  MG_HIP (hipStreamSynchronize (st));
  if (nBad) *nBad = bad;
  gInfDiag[0] += n; gInfDiag[2] += text; ++gInfDiag[3];
  return MG_OK;
}
extern "C" size_t mgInflateWorkBytes (U32 n) { return (size_t) n * (sizeof (MgGzMember) + 4) + 4; }

extern "C" MgStatus mgInflateMembersDevice (const U8 *dComp, U64 compBytes, const MgGzMember *members, U32 n, U8 *dOut, U64 outBytes, U32 *status, U32 *nBad, void *stream)
{
  mgInflateDiagReset ();
  if (nBad) *nBad = 0;
  if (!n) return MG_OK;
  if (!members || !dComp || !dOut) { mgSetError ("mgInflateMembersDevice: null argument"); return MG_ERR_ARG; }
  if (infCheck (members, n, compBytes, outBytes)) return MG_ERR_ARG;          /* refused before the device is touched */
  const MgStatus ok = mgEnsureDevice (); if (ok != MG_OK) return ok;
  MgDevScratch scratch ("mgInflateMembersDevice");
  U8 *dWork = 0;
  if (scratch.get (&dWork, mgInflateWorkBytes (n))) return MG_ERR_HIP;
  return mgInflateRun (dComp, compBytes, members, n, dOut, outBytes, dWork, status, nBad, stream);
}

/* the decoder's host compile: one member, as the kernel does it, on the calling thread.  A test hook (as mgIterScanHost is) */
extern "C" int mgInflateMemberHost (const U8 *comp, U32 cLen, U8 *out, U32 uLen, U32 crc, U32 *status, U64 stats8[8])
{
  MgInfTables T;
  if (stats8) memset (stats8, 0, 8 * sizeof (U64));
  if ((!comp && cLen) || (!out && uLen)) { mgSetError ("mgInflateMemberHost: null argument"); return -1; }
  const U32 st = mgInfMember (comp, cLen, out, uLen, crc, &T, (uint64_t *) stats8);
  if (status) *status = st;
  return 0;
}
