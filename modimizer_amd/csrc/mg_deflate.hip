/* mg_deflate.hip — text blocks of at most 65280 bytes deflated into BGZF members on the device: the kernel, the gather that packs the members,
 * mgDeflateBlocksDevice and the host compile of the encoder (mgDeflateBlockHost).  The encoder itself is mg_deflate_core.h, written once for
 * both sides; what is parallel and what is serial in it is said there.
 *
 * Shape: one workgroup of FOUR waves a block; workgroup w of the launch takes blocks w, w + grid, ..
 *   - Why four waves and not one (as the inflate kernel has).  The encoder's work area is 30 KiB of LDS, so a CU's 160 KiB hold five blocks
 *     whatever the workgroup's size: with one wave a block a CU would run 5 waves, with four it runs 20, and the parallel phases -- candidate
 *     lookup and match verification, the byte histogram, the bit emission, the zeroing -- are wide enough (1024 positions a step, thousands of
 *     tokens) to use 256 lanes.  (The compiler's 133 VGPRs allow 3 waves a SIMD, so a CU runs three blocks, 12 waves: the registers bind
 *     before LDS does.)  The serial phases (the greedy walk: the first wave; the code construction: lane 0) leave the other lanes at the
 *     barrier; the other workgroups of the CU run meanwhile.
 *   - LDS: the hash table (16 KiB), a step's candidates / tokens-to-be (4 KiB), histograms, code tables, the sort's keys: MgDefWork.
 *   - Device scratch (MgDeflateWork owns it): the token list, up to 65280 words, is too large for LDS: a slice per WORKGROUP; the members are
 *     written into 64 KiB slots, one per BLOCK; the members' lengths.  A device-wide exclusive scan of the lengths (mgExclusiveScan) gives
 *     every member its place, and the gather kernel packs them into the caller's buffer in order: nothing but the file's bytes leaves.
 *   - Hand-offs through memory inside a workgroup -- lane 0's tokens read by every lane, zeroed words OR-ed by others -- have __syncthreads ()
 *     between them: a workgroup-scope release, the barrier, an acquire.  Words of the slot that lanes share are only ever OR-ed (atomicOr). */
#include <string.h>
#include <stdlib.h>
#include "mg_common.h"
#include "mg_internal.h"
#include "mg_devsort.h"
#include "mg_deflate_core.h"

#define DEF_THREADS 256
#define DEF_GRID_MAX 1280u                               /* workgroups of a launch: 5 a CU on 256 CUs; each owns a token slice of 255 KiB */
#define DEF_LAUNCH_MAX 32768u                            /* blocks of a launch: their members' lengths sum to less than 2^32 (the scan's words) */
static_assert (DEF_THREADS <= MGD_MAX_LANES && DEF_THREADS >= 64, "the core's lane table; its greedy walk is the first wave's");

__global__ __launch_bounds__ (DEF_THREADS)
void mgDeflateKernel (const U8 *__restrict__ text, const MgGzBlock *__restrict__ blocks, U32 n, U8 *slots, U32 *tokens, U32 *lens)
{
  __shared__ MgDefWork W;
  U32 *mine = tokens + (size_t) blockIdx.x * MGD_BLOCK_MAX;
  for (U32 m = blockIdx.x ; m < n ; m += gridDim.x)
    { const MgGzBlock b = blocks[m];
      const U32 len = mgDefMember (text + b.uOff, b.uLen, slots + (size_t) m * MGD_SLOT, mine, &W, threadIdx.x, DEF_THREADS, 0);
      if (threadIdx.x == 0) lens[m] = len;
    }
}

/* member m's bytes from its slot to out[place[m] ..): the destination is byte-packed, so bytes */
__global__ __launch_bounds__ (DEF_THREADS)
void mgDeflateGatherKernel (const U8 *__restrict__ slots, const U32 *__restrict__ lens, const U32 *__restrict__ place, U32 n, U8 *out)
{
  for (U32 m = blockIdx.x ; m < n ; m += gridDim.x)
    { const U32 len = lens[m] < MGD_SLOT ? lens[m] : MGD_SLOT;
      const U8 *src = slots + (size_t) m * MGD_SLOT;
      U8 *dst = out + place[m];
      for (U32 i = threadIdx.x ; i < len ; i += DEF_THREADS) dst[i] = src[i];
    }
}

static thread_local U64 gDefDiag[4];                     /* blocks deflated on the device, text bytes in, file bytes out, kernel launches */
extern "C" void mgDeflateDiag (U64 out4[4]) { memcpy (out4, gDefDiag, sizeof (gDefDiag)); }
extern "C" void mgDeflateDiagReset (void) { memset (gDefDiag, 0, sizeof (gDefDiag)); }

struct MgDeflateWork {
  MgDevBuf<U8> slots; MgDevBuf<U32> tokens, lens; MgDevBuf<MgGzBlock> blocks;
  std::vector<U32> hLens;
  void drop () { slots.drop (); tokens.drop (); lens.drop (); blocks.drop (); }
};
extern "C" MgDeflateWork *mgDeflateWorkNew (void) { return new MgDeflateWork; }
extern "C" void mgDeflateWorkFree (MgDeflateWork *w) { if (w) { w->drop (); delete w; } }

/* slot: the output bytes asked for per block: 65536 of the public call's callers; 0: what a member can be at most -- the stored form, the block's bytes + 31 */
static int defCheck (const MgGzBlock *blocks, U32 n, U64 textBytes, U64 outBytes, U32 slot)
{
  U64 need = (U64) n * slot;
  if (outBytes < need) { mgSetError ("mgDeflateBlocksDevice: %llu bytes of output for %u blocks: 65536 a block", (unsigned long long) outBytes, n); return -1; }
  for (U32 i = 0 ; i < n && !slot ; ++i) need += (U64) blocks[i].uLen + 31;
  if (outBytes < need) { mgSetError ("mgDeflateBlocksDevice: %llu bytes of output, %llu needed", (unsigned long long) outBytes, (unsigned long long) need); return -1; }
  for (U32 i = 0 ; i < n ; ++i)
    { const MgGzBlock &b = blocks[i];
      if (b.uLen > MGD_BLOCK_MAX) { mgSetError ("mgDeflateBlocksDevice: block %u of %u bytes: at most %u", i, b.uLen, MGD_BLOCK_MAX); return -1; }
      if (b.uOff > textBytes || b.uLen > textBytes - b.uOff) { mgSetError ("mgDeflateBlocksDevice: block %u leaves its buffer", i); return -1; }
    }
  return 0;
}

extern "C" MgStatus mgDeflateRun (MgDeflateWork *w, const U8 *dText, U64 textBytes, const MgGzBlock *blocks, U32 n, U8 *dOut, U64 outBytes, U64 *memberOff, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  if (memberOff) memberOff[0] = 0;
  if (!n) return MG_OK;
  if (!blocks || !dOut || !memberOff || (!dText && textBytes)) { mgSetError ("mgDeflateBlocksDevice: null argument"); return MG_ERR_ARG; }
  if (defCheck (blocks, n, textBytes, outBytes, 0)) return MG_ERR_ARG;
  const char *what = "mgDeflateBlocksDevice";
  U64 done = 0;                                          /* bytes packed so far */
  for (U32 at = 0 ; at < n ; at += DEF_LAUNCH_MAX)
    { const U32 k = n - at < DEF_LAUNCH_MAX ? n - at : DEF_LAUNCH_MAX, grid = k < DEF_GRID_MAX ? k : DEF_GRID_MAX;
      MgStatus s;
      if ((s = w->slots.reserve ((size_t) k * MGD_SLOT, (size_t) k * MGD_SLOT, what)) || (s = w->tokens.reserve ((size_t) grid * MGD_BLOCK_MAX, (size_t) grid * MGD_BLOCK_MAX, what))
          || (s = w->lens.reserve (2 * (size_t) k, 2 * (size_t) k, what)) || (s = w->blocks.reserve (k, k, what))) return s;
      U32 *dLens = w->lens.p, *dPlace = dLens + k, total = 0;
      U64 text = 0;
      for (U32 i = 0 ; i < k ; ++i) text += blocks[at + i].uLen;
      MG_HIP (hipMemcpyAsync (w->blocks.p, blocks + at, (size_t) k * sizeof (MgGzBlock), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL (mgDeflateKernel, dim3 (grid), dim3 (DEF_THREADS), 0, st, dText, w->blocks.p, k, w->slots.p, w->tokens.p, dLens);
      MG_HIP (hipGetLastError ());
      { MgDevScratch scratch (what);
        if ((s = mgExclusiveScan (scratch, dLens, dPlace, k, st, &total))) return s;      /* (waits for the stream) */
        if (total > (U64) k * MGD_SLOT || done + total > outBytes) { mgSetError ("mgDeflateBlocksDevice: %u bytes of members from %u blocks", total, k); return MG_ERR_HIP; }
        hipLaunchKernelGGL (mgDeflateGatherKernel, dim3 (grid), dim3 (DEF_THREADS), 0, st, w->slots.p, dLens, dPlace, k, dOut + done);
        MG_HIP (hipGetLastError ());
        w->hLens.resize (k);
        MG_HIP (hipMemcpyAsync (w->hLens.data (), dLens, (size_t) k * 4, hipMemcpyDeviceToHost, st));
        MG_HIP (hipStreamSynchronize (st));
      }
      for (U32 i = 0 ; i < k ; ++i) { done += w->hLens[i]; memberOff[at + i + 1] = done; }
      gDefDiag[0] += k; gDefDiag[1] += text; gDefDiag[2] += total; ++gDefDiag[3];
    }
  return MG_OK;
}

extern "C" MgStatus mgDeflateBlocksDevice (const U8 *dText, U64 textBytes, const MgGzBlock *blocks, U32 n, U8 *dOut, U64 outBytes, U64 *memberOff, void *stream)
{
  mgDeflateDiagReset ();
  if (memberOff) memberOff[0] = 0;
  if (!n) return MG_OK;
  if (!blocks || !dOut || !memberOff || (!dText && textBytes)) { mgSetError ("mgDeflateBlocksDevice: null argument"); return MG_ERR_ARG; }
  if (defCheck (blocks, n, textBytes, outBytes, MGD_SLOT)) return MG_ERR_ARG;  /* refused before the device is touched */
  const MgStatus ok = mgEnsureDevice (); if (ok != MG_OK) return ok;
  MgDeflateWork w;
  const MgStatus s = mgDeflateRun (&w, dText, textBytes, blocks, n, dOut, outBytes, memberOff, stream);
  if (s != MG_OK) (void) hipStreamSynchronize ((hipStream_t) stream);
  w.drop ();
  return s;
}

/* the encoder's host compile: one block, as a workgroup does it, on the calling thread as lane 0 of 1.  A test hook (as mgInflateMemberHost is) */
extern "C" int mgDeflateBlockHost (const U8 *text, U32 uLen, U8 *out, U32 *outLen, U64 stats8[8])
{
  if (stats8) memset (stats8, 0, 8 * sizeof (U64));
  if (outLen) *outLen = 0;
  if ((!text && uLen) || !out || !outLen) { mgSetError ("mgDeflateBlockHost: null argument"); return -1; }
  if (uLen > MGD_BLOCK_MAX) { mgSetError ("mgDeflateBlockHost: a block of %u bytes: at most %u", uLen, MGD_BLOCK_MAX); return -1; }
  MgDefWork *W = (MgDefWork *) malloc (sizeof (MgDefWork));
  U32 *tokens = (U32 *) malloc ((size_t) (uLen ? uLen : 1) * 4);
  int rc = -1;
  if (W && tokens) { *outLen = mgDefMember (text, uLen, out, tokens, W, 0, 1, (uint64_t *) stats8); rc = 0; }
  else mgSetError ("mgDeflateBlockHost: out of memory");
  free (W); free (tokens);
  return rc;
}
