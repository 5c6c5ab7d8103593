/* mg_modutils.hip — the rest of modutils on the device: -x (modutils.c:33-51 with is10x), -s / -sM (modutils.c:205-219) and the counters
 * of the set summary (modset.c:130-153).
 *
 * -x   Records are numbered from 1 through a file; a record with an odd number loses its first 23 bases (the 10x barcode and UMI) as the
 *      reader delivers them, a shorter one becomes an empty read (the reference aborts on it, seqhash.c:156).  A batch is trimmed where
 *      it lies, 2-bit packed (mgTrim10xDevice):
 *        skip     per record: 23 (or its whole length) if its number is odd, else 0;
 *        scan     the skips' exclusive sum (mgExclusiveScan: 32 bits, so a batch of more than (2^32 - 1) / 23 records is refused);
 *        offsets  out[i] = in[i] - cumSkip[i];
 *        gather   a lane per output word: the record of its first base by an upper-bound search in the new offsets (empty records fall
 *                 away), then record after record, each piece shifted out of two source words.
 *      The device text parser's sink (mg_textgpu.hip) and mgAddSequenceBatch10x put it between the packed batch and mgAddReadsDevice.
 *
 * -s   One kernel walks the table's slots as the histogram does: per entry d = min (65535, baseDepth + pending), the class by the
 *      reference's else-if chain, info[] changed on the device copy the call uploaded and copied back.  Nothing is folded: the table's
 *      pending counts, syncedMax and live histogram are what they were, and no byte of value[] or depth[] crosses the link.
 *
 * summary   mgTableHistogram's 65536 bins and four tallies of info[] & 3: 65540 counters come back, mg_host.c prints the lines.
 */
#include <string.h>
#include "mg_common.h"
#include "mg_internal.h"
#include "mg_table.h"
#include "mg_devsort.h"
#include "mg_xfer.h"

#define MG_10X_SKIP 23u                                  /* modutils.c:44 */

/* ======================================================================================== */
/* -x: the trim                                                                               */

/* skip[i] for i < nReads, skip[nReads] = 0 (so that the scan over nReads + 1 leaves the total skip in cum[nReads]) */
__global__ void mgTrimSkipKernel (const U64 *__restrict__ off, U32 nReads, U64 firstOrdinal, U32 *__restrict__ skip)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= nReads ; i += (U64) gridDim.x * blockDim.x)
    { U32 s = 0;
      if (i < nReads && ((firstOrdinal + i) & 1))
        { const U64 len = off[i + 1] - off[i]; s = len < MG_10X_SKIP ? (U32) len : MG_10X_SKIP; }
      skip[i] = s;
    }
}

__global__ void mgTrimOffsetsKernel (const U64 *__restrict__ off, const U32 *__restrict__ cum, U32 nReads, U64 *__restrict__ offOut)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= nReads ; i += (U64) gridDim.x * blockDim.x) offOut[i] = off[i] - cum[i];
}

/* word j of the trimmed batch (first base in the top bits, mgPackKernel); words past the last base are zero.  Base p of the output lies
   in the record r with offOut[r] <= p < offOut[r + 1] and is base p + (off[r + 1] - offOut[r + 1]) of the input: what was cut up to and
   including r's own barcode.  nWordsIn: words of `packed` that may be read */
__global__ __launch_bounds__ (256)
void mgTrimGatherKernel (const U32 *__restrict__ packed, U64 nWordsIn, const U64 *__restrict__ off, const U64 *__restrict__ offOut, U32 nReads,
                         U64 totalOut, U32 *__restrict__ out, U64 nWordsOut)
{
  for (U64 j = (U64) blockIdx.x * blockDim.x + threadIdx.x ; j < nWordsOut ; j += (U64) gridDim.x * blockDim.x)
    { U32 wv = 0;
      U64 p = j * 16;
      if (p < totalOut)
        { U32 lo = 0, hi = nReads;                                         /* the first r' with offOut[r'] > p: in 1 .. nReads, as offOut[0] = 0 and offOut[nReads] = totalOut */
          while (lo < hi) { const U32 mid = lo + (hi - lo) / 2; if (offOut[mid] > p) hi = mid; else lo = mid + 1; }
          U32 r = lo - 1;
          U32 filled = 0;
          while (filled < 16 && p < totalOut && r < nReads)                /* (r < nReads, n != 0 and the guarded loads hold for offsets that ascend from 0; others end the walk) */
            { const U64 end = offOut[r + 1];
              const U32 room = 16 - filled, n = end - p < room ? (U32) (end - p) : room;
              if (!n) break;
              const U64 src = p + (off[r + 1] - end);
              const U64 sw = src >> 4; const U32 sh = 2u * (U32) (src & 15);
              const U64 two = ((U64) (sw < nWordsIn ? packed[sw] : 0u) << 32) | (sw + 1 < nWordsIn ? packed[sw + 1] : 0u);
              U32 v = (U32) ((two << sh) >> 32);                           /* the 16 bases from src on */
              if (n < 16) v &= ~(0xffffffffu >> (2 * n));
              wv |= v >> (2 * filled);
              p += n; filled += n;
              if (p == end) { ++r; while (r < nReads && offOut[r + 1] == p) ++r; }      /* on to the next record that holds a base */
            }
        }
      out[j] = wv;
    }
}

extern "C" MgStatus mgTrim10xDevice (const U32 *dPacked, U64 totalBases, const U64 *dOff, U32 nReads, U64 firstOrdinal,
                                     U32 *dPackedOut, U64 *dOffOut, U64 *totalOut, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  MgStatus s = mgEnsureDevice (); if (s) return s;
  if (totalOut) *totalOut = 0;
  if (!dOff || !dOffOut || !dPackedOut || (totalBases && !dPacked)) { mgSetError ("mgTrim10xDevice: null argument"); return MG_ERR_ARG; }
  if ((U64) nReads > 0xffffffffull / MG_10X_SKIP)
    { mgSetError ("mgTrim10xDevice: %u records in one batch (their skips are summed in 32 bits: at most %u)", nReads, (U32) (0xffffffffull / MG_10X_SKIP)); return MG_ERR_ARG; }
  MgDevScratch scratch ("mgTrim10xDevice");
  U32 *dSkip, *dCum;
  const U64 n1 = (U64) nReads + 1;
  if (scratch.get (&dSkip, n1) || scratch.get (&dCum, n1)) return MG_ERR_HIP;
  MG_LAUNCH (MG_K_TRIM_OFFSETS, st, mgTrimSkipKernel, dim3 (mgGrid (n1)), dim3 (256), 0, st, dOff, nReads, firstOrdinal, dSkip);
  MG_HIP (hipGetLastError ());
  U32 cut = 0;
  if ((s = mgExclusiveScan (scratch, dSkip, dCum, n1, st, &cut))) return s;
  if ((U64) cut > totalBases) { mgSetError ("mgTrim10xDevice: the read offsets do not end at totalBases"); return MG_ERR_ARG; }
  const U64 outBases = nReads ? totalBases - cut : 0;
  const U64 nWordsIn = (U64) mgPackedWords (totalBases), nWordsOut = (U64) mgPackedWords (outBases);
  MG_LAUNCH (MG_K_TRIM_OFFSETS, st, mgTrimOffsetsKernel, dim3 (mgGrid (n1)), dim3 (256), 0, st, dOff, dCum, nReads, dOffOut);
  MG_LAUNCH (MG_K_TRIM_GATHER, st, mgTrimGatherKernel, dim3 (mgGrid (nWordsOut, 256, 16384)), dim3 (256), 0, st,
             dPacked, nWordsIn, dOff, dOffOut, nReads, outBases, dPackedOut, nWordsOut);
  MG_HIP (hipGetLastError ());
  MG_HIP (hipStreamSynchronize (st));                    /* (the scratch goes when this returns) */
  if (totalOut) *totalOut = outBases;
  return MG_OK;
}

/* the census of the calling thread's last mgAddSequenceFile10x (or of the mgAddSequenceBatch10x calls since) */
static thread_local U64 gTenX[4];
extern "C" void mgAdd10xDiag (U64 out4[4]) { for (int i = 0 ; i < 4 ; ++i) out4[i] = gTenX[i]; }
extern "C" void mgAdd10xDiagReset (void) { memset (gTenX, 0, sizeof (gTenX)); }
extern "C" void mgAdd10xDiagHostLeg (void) { gTenX[3] = 1; }
/* a batch of nReads records from number firstOrdinal on went through the trim and lost `dropped` bases */
extern "C" void mgAdd10xDiagBatch (U32 nReads, U64 firstOrdinal, U64 dropped)
{ ++gTenX[0]; gTenX[1] += (firstOrdinal & 1) ? ((U64) nReads + 1) / 2 : (U64) nReads / 2; gTenX[2] += dropped; }

/* mgAddSequenceBatch with the batch's records numbered from firstOrdinal: uploaded and packed, trimmed, added.  Hashes added, or -1 */
extern "C" int64_t mgAddSequenceBatch10x (Modset *ms, const char *bases, const int64_t *readOffsets, int nReads, uint64_t firstOrdinal)
{
  if (mgEnsureDevice ()) return -1;
  if (nReads <= 0) return 0;
  const U64 total = (U64) readOffsets[nReads];
  MgDevScratch scratch ("mgAddSequenceBatch10x");
  U32 *dP, *dPOut; U64 *dOff, *dOffOut;
  const size_t nw = mgPackedWords (total);
  if (scratch.get (&dP, nw) || scratch.get (&dPOut, nw) || scratch.get (&dOff, (size_t) nReads + 1) || scratch.get (&dOffOut, (size_t) nReads + 1)) return -1;
  if (hipMemcpyAsync (dOff, readOffsets, ((size_t) nReads + 1) * 8, hipMemcpyHostToDevice, 0) != hipSuccess || mgUploadPack (bases, total, dP, 0) != MG_OK)
    return mgFailedWith ("mgAddSequenceBatch10x: copy to the device failed");
  U64 outBases = 0, nHash = 0;
  if (mgTrim10xDevice (dP, total, dOff, (U32) nReads, firstOrdinal, dPOut, dOffOut, &outBases, 0)) return -1;
  mgAdd10xDiagBatch ((U32) nReads, firstOrdinal, total - outBases);
  if (mgAddReadsDevice (ms, dPOut, outBases, dOffOut, (U32) nReads, &nHash, 0) != MG_OK || hipStreamSynchronize (0) != hipSuccess) return -1;
  return (int64_t) nHash;
}

/* ======================================================================================== */
/* -s / -sM                                                                                   */

/* modutils.c:209-212 in int arithmetic: the chain decides, whatever the thresholds' order */
__host__ __device__ __forceinline__ U32 mgCopyClass (int d, int c1, int c2, int cM) { return d < c1 ? 0u : d < c2 ? 1u : d < cM ? 2u : 3u; }

/* onlyM: -sM (info |= 3 where d >= cM); else -s.  Every index sits in one slot, so every info byte has one writer; entry 0 has none */
__global__ __launch_bounds__ (256)
void mgSetCopyKernel (const MgSlot *__restrict__ slots, U32 nBuckets, const U32 *__restrict__ occ, U32 R, const U16 *__restrict__ baseDepth, U32 max,
                      int c1, int c2, int cM, int onlyM, U8 *__restrict__ info)
{
  for (U32 bk = blockIdx.x ; bk < nBuckets ; bk += gridDim.x)
    { if (!occ[bk]) continue;
      const MgSlot *base = slots + (U64) bk * R;
      for (U32 i = threadIdx.x ; i < R ; i += blockDim.x)
        { const uint4 v = *reinterpret_cast<const uint4 *> (&base[i]);
          if (!(v.x | v.y) || !mgIsAssigned (v.z)) continue;
          const U32 idx = v.z & ~MG_ASSIGNED;
          if (!idx || idx > max) continue;
          U32 d = (baseDepth ? (U32) baseDepth[idx] : 0u) + v.w;            /* baseDepth == 0: known to be all zero */
          if (d > 0xffffu || d < v.w) d = 0xffffu;
          const U8 f = info[idx];
          if (onlyM) { if ((int) d >= cM) info[idx] = (U8) (f | 3u); }
          else info[idx] = (U8) ((f & 0xfcu) | mgCopyClass ((int) d, c1, c2, cM));
        }
    }
}

static thread_local int gSetCopyPath = -1;
extern "C" int mgModsetSetCopyPath (void) { return gSetCopyPath; }

/* the set's info[0 .. max] on the device (scratch's), as the host holds it */
static MgStatus mgInfoUpload (MgDevScratch &scratch, Modset *ms, U32 max, U8 **dInfo)
{
  MgStatus s;
  if ((U64) max + 1 > ms->size) { mgSetError ("the set's host arrays hold %u entries, its device table %u", ms->size, max); return MG_ERR_ARG; }
  if ((s = scratch.get (dInfo, (size_t) max + 1 + 16))) return s;
  MG_HIP (hipMemset (*dInfo + max + 1, 0, 16));
  return mgXferH2DSparse (*dInfo, ms->info, (size_t) max + 1);
}

static int mgSetCopyRun (Modset *ms, int c1, int c2, int cM, int onlyM)
{
  gSetCopyPath = -1;
  if (!ms) { mgSetError ("null Modset"); return -1; }
  MgTable *t = 0;
  if (mgModsetTableForPass (ms, &t)) return -1;
  if (!t)                                                /* a set without a device table: the reference's loop */
    { for (U32 u = 1 ; u <= ms->max ; ++u)
        { const int d = ms->depth[u];
          if (onlyM) { if (d >= cM) ms->info[u] |= 3; }
          else ms->info[u] = (U8) ((ms->info[u] & 0xfc) | mgCopyClass (d, c1, c2, cM));
        }
      gSetCopyPath = 1;
      return 0;
    }
  gSetCopyPath = 0;
  if (!t->max) return 0;
  hipStream_t st = 0;
  MgDevScratch scratch (onlyM ? "mgModsetSetCopyM" : "mgModsetSetCopy");
  U8 *dInfo;
  const U32 NB = 1u << t->log2NB;
  if (mgInfoUpload (scratch, ms, t->max, &dInfo)) { gSetCopyPath = -1; return -1; }
  MG_LAUNCH (MG_K_SETCOPY, st, mgSetCopyKernel, dim3 (NB < 8192 ? NB : 8192), dim3 (256), 0, st,
             t->slots, NB, t->occ, t->R, t->baseZero ? (const U16 *) 0 : t->baseDepth, t->max, c1, c2, cM, onlyM, dInfo);
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st) != hipSuccess || mgXferD2H (ms->info + 1, dInfo + 1, t->max, MG_XFER_COPY))
    { gSetCopyPath = -1; return mgFailedWith ("set copy on the device failed"); }
  return 0;
}

extern "C" int mgModsetSetCopy (Modset *ms, int copy1min, int copy2min, int copyMmin) { return mgSetCopyRun (ms, copy1min, copy2min, copyMmin, 0); }
extern "C" int mgModsetSetCopyM (Modset *ms, int copyMmin) { return mgSetCopyRun (ms, 0, 0, copyMmin, 1); }

/* ======================================================================================== */
/* the summary's counters                                                                     */

/* tally[c] += entries 1 .. max with (info & 3) == c; info is read 16 bytes a lane (the array starts on an allocation's boundary and
   has 16 bytes of zero behind entry max) */
__global__ __launch_bounds__ (256)
void mgCopyTallyKernel (const U8 *__restrict__ info, U32 max, unsigned long long *__restrict__ tally)
{
  __shared__ U32 lds[4];
  const U64 nChunks = ((U64) max + 16) / 16;              /* bytes 0 .. max */
  U32 n1 = 0, n2 = 0, n3 = 0, nAll = 0;
  for (U64 c = (U64) blockIdx.x * blockDim.x + threadIdx.x ; c < nChunks ; c += (U64) gridDim.x * blockDim.x)
    { const uint4 v = *reinterpret_cast<const uint4 *> (info + c * 16);
      const U32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
      for (int q = 0 ; q < 4 ; ++q)
        { const U64 b0 = c * 16 + (U64) q * 4;              /* the word's first entry */
          U32 valid = 0x01010101u;                         /* bit 8 b: byte b is an entry in 1 .. max */
          if (b0 + 3 > max) valid = b0 > max ? 0u : valid & (0xffffffffu >> (8 * (b0 + 3 - max)));
          if (!b0) valid &= ~1u;
          const U32 x = w[q], a = x & valid, b = (x >> 1) & valid;
          n1 += (U32) __popc (a & ~b); n2 += (U32) __popc (b & ~a); n3 += (U32) __popc (a & b); nAll += (U32) __popc (valid);
        }
    }
  const U32 t1 = mgBlockReduce<256, MgSum> (n1, lds), t2 = mgBlockReduce<256, MgSum> (n2, lds), t3 = mgBlockReduce<256, MgSum> (n3, lds),
            tA = mgBlockReduce<256, MgSum> (nAll, lds);
  if (threadIdx.x == 0 && tA)
    { atomicAdd (&tally[0], (unsigned long long) (tA - t1 - t2 - t3));
      if (t1) atomicAdd (&tally[1], (unsigned long long) t1);
      if (t2) atomicAdd (&tally[2], (unsigned long long) t2);
      if (t3) atomicAdd (&tally[3], (unsigned long long) t3);
    }
}

/* counters[0 .. 65536): entries by depth; [65536 .. 65540): by copy class.  1: the set has no device table */
extern "C" int mgSummaryCountersDevice (Modset *ms, U64 *counters)
{
  MgTable *t = 0;
  if (mgModsetTableForPass (ms, &t)) return -1;
  if (!t) return 1;
  memset (counters, 0, 65540 * sizeof (U64));
  if (!t->max) return 0;
  hipStream_t st = 0;
  MgDevScratch scratch ("mgModsetSummaryDevice");
  U8 *dInfo; U64 *dOut;
  if (scratch.get (&dOut, 65540) || mgInfoUpload (scratch, ms, t->max, &dInfo)) return -1;
  if (hipMemsetAsync (dOut, 0, 65540 * sizeof (U64), st) != hipSuccess || mgTableHistogram (t, dOut, st)) return mgFailedWith ("summary on the device failed");
  MG_LAUNCH (MG_K_COPY_TALLY, st, mgCopyTallyKernel, dim3 (mgGrid (((U64) t->max + 16) / 16, 256, 2048)), dim3 (256), 0, st, dInfo, t->max, (unsigned long long *) dOut + 65536);
  if (hipGetLastError () != hipSuccess || hipMemcpyAsync (counters, dOut, 65540 * sizeof (U64), hipMemcpyDeviceToHost, st) != hipSuccess
      || hipStreamSynchronize (st) != hipSuccess) return mgFailedWith ("summary on the device failed");
  return 0;
}
