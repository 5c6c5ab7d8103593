/* mg_find.hip — K3: lookups in the device modset table (mg_table.hip: layout).  Direct probes in ordinal order, dense or from the scan's
 * segments; and the partitioned lookups, which send the batch through the build's partition passes (mg_part.hip) first.  The builds are mg_tableadd.hip. */
#include "mg_table.h"

/* ---- the read-only probe walk: every lookup kernel's ----
 * A view of one bucket's slots says how slot i is read (read), what it is compared by (tag: the key, or what stands for it;
 * 0 = empty) and which index it answers on a hit (index). */
struct MgTableSlots            /* the table's own 16-byte slots, in global memory */
{ const MgSlot *s;
  typedef uint4 Word;
  __device__ __forceinline__ Word read (U32 i) const { return *reinterpret_cast<const uint4 *> (&s[i]); }
  __device__ __forceinline__ U64 tag (const Word &w) const { return mgKeyOf (w); }
  __device__ __forceinline__ U32 index (U32, const Word &w) const { return mgIndexOf (w.z); }
};
struct MgImageSlots            /* a bucket's image in LDS: keys and indices apart */
{ const unsigned long long *sKey; const U32 *sIdx;
  typedef unsigned long long Word;
  __device__ __forceinline__ Word read (U32 i) const { return sKey[i]; }
  __device__ __forceinline__ U64 tag (Word w) const { return w; }
  __device__ __forceinline__ U32 index (U32 i, Word) const { return sIdx[i]; }
};
struct MgImageWords8           /* the same from the 8-byte copy (mgTablePack8Kernel): (key's low bits + 1) << 31 | index */
{ const unsigned long long *sW;
  typedef unsigned long long Word;
  __device__ __forceinline__ Word read (U32 i) const { return sW[i]; }
  __device__ __forceinline__ U64 tag (Word w) const { return w >> 31; }
  __device__ __forceinline__ U32 index (U32, Word w) const { return (U32) w & 0x7fffffffu; }
};
/* Linear probing, wrapping inside the bucket: from slot `at` on until the slot that holds `want` (its index is the answer) or an empty
 * one, over at most R slots in all (then, as at an empty slot, 0).  probes: slots of the walk the caller has looked at itself. */
template <class Slots>
__device__ __forceinline__ U32 mgProbeFind (const Slots &sl, U32 at, U32 R, U64 want, U32 probes = 0)
{
  for ( ; probes < R ; ++probes)
    { const typename Slots::Word w = sl.read (at);
      const U64 cur = sl.tag (w);
      if (cur == want) return sl.index (at, w);
      if (cur == 0) break;
      at = mgNextSlot (at, R);
    }
  return 0;
}

/* The query's lookups.  MG_FIND_PER k-mers per thread and step: all the k-mer loads, then all the first probes (one
 * 16-byte load each: key and index together), land before anything is stored -- a loop of "load, probe, store" made
 * every store wait for the one before it; only the probes that hit another k-mer's slot walk on.  CHECK_OCC = false
 * when every bucket's bytes are defined (mgTableClean has zeroed the never-written ones): no dependent load in front. */
#ifndef MG_FIND_PER
#define MG_FIND_PER 1
#endif
template <bool CHECK_OCC>
__global__ __launch_bounds__ (256)
void mgTableFindKernel (const MgSlot *__restrict__ slots, const U32 *__restrict__ occ, MgGeom g,
                        const U64 *__restrict__ kmer, U64 n, U32 *__restrict__ out)
{
  MG_BUILD_PRIO ();
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for (U64 o0 = (U64) blockIdx.x * blockDim.x + threadIdx.x ; o0 < n ; o0 += stride * MG_FIND_PER)
    { U64 km[MG_FIND_PER], key[MG_FIND_PER], base[MG_FIND_PER]; U32 at[MG_FIND_PER], res[MG_FIND_PER]; bool live[MG_FIND_PER];
      uint4 v[MG_FIND_PER];
#pragma unroll
      for (int j = 0 ; j < MG_FIND_PER ; ++j) { const U64 o = o0 + (U64) j * stride; km[j] = o < n ? __builtin_nontemporal_load (&kmer[o]) : 0; }
#pragma unroll
      for (int j = 0 ; j < MG_FIND_PER ; ++j)
        { const U64 m = mgMixK (km[j], g.kbits);
          const U32 bkt = mgBucketOfM (m, g);
          key[j] = m + 1; base[j] = (U64) bkt * g.R; at[j] = mgHomeOfM (m, g);
          live[j] = o0 + (U64) j * stride < n;
          if (CHECK_OCC && live[j] && !occ[bkt]) live[j] = false;      /* never written: its bytes are undefined */
          v[j] = make_uint4 (0, 0, 0, 0);
          if (live[j]) v[j] = *reinterpret_cast<const uint4 *> (&slots[base[j] + at[j]]);
        }
#pragma unroll
      for (int j = 0 ; j < MG_FIND_PER ; ++j) asm volatile ("" : "+v" (v[j].x), "+v" (v[j].y), "+v" (v[j].z));
#pragma unroll
      for (int j = 0 ; j < MG_FIND_PER ; ++j)
        { const U64 cur = mgKeyOf (v[j]);
          res[j] = cur == key[j] ? mgIndexOf (v[j].z) : 0;
          if (live[j] && cur != 0 && cur != key[j]) res[j] = mgProbeFind (MgTableSlots { slots + base[j] }, mgNextSlot (at[j], g.R), g.R, key[j], 1);   /* met another k-mer's slot: walk on */
        }
#pragma unroll
      for (int j = 0 ; j < MG_FIND_PER ; ++j) { const U64 o = o0 + (U64) j * stride; if (o < n) __builtin_nontemporal_store (res[j], &out[o]); }
    }
}

/* the same lookups for k-mers that still sit in the scan's segments: a wave walks a contiguous range of rows of 64
 * ordinals with a segment cursor (see MgSegCursor) */
__global__ __launch_bounds__ (256)
void mgTableFindSegKernel (const MgSlot *__restrict__ slots, MgGeom g, const MgSegSrc src, U64 n, U64 rowsPerWave, U32 *__restrict__ out)
{
  MG_BUILD_PRIO ();
  const int lane = threadIdx.x & 63;
  const U64 wave = (U64) blockIdx.x * 4 + (U32) __builtin_amdgcn_readfirstlane ((int) (threadIdx.x >> 6));
  const U64 nRows = (n + 63) / 64;
  U64 row = wave * rowsPerWave, rEnd = row + rowsPerWave;
  if (rEnd > nRows) rEnd = nRows;
  if (row >= rEnd) return;
  MgSegCursor cur;
  mgSegCursorAt (src, mgSegOfOrdinal (src, row * 64), &cur);
  for ( ; row < rEnd ; ++row)
    { const U64 o0 = row * 64, o = o0 + (U64) lane, last = o0 + 63 < n ? o0 + 63 : n - 1;
      mgSegCursorSeek (src, &cur, o0);
      const U64 *at = mgSegAddr (src, cur, o < n ? o : last, last);
      if (o >= n) continue;
      const U64 m = mgMixK (__builtin_nontemporal_load (at), g.kbits), key = m + 1;
      const U64 base = (U64) mgBucketOfM (m, g) * g.R;
      __builtin_nontemporal_store (mgProbeFind (MgTableSlots { slots + base }, mgHomeOfM (m, g), g.R, key), &out[o]);
    }
}

/* ======================================================================================== */
/* Partitioned lookups (the modmap query path on a table far larger than the caches, round 4).  A lookup in ordinal order
 * is one random 64-byte line out of a 2 GB table: 35 G lookups/s, the chip's rate for that footprint.  Here the batch's
 * modimizers go through the FIRST partition pass of the build (by the top bits of the mixed k-mer, straight from the scan's
 * segments, the digit counts made by the scan); a bin's lookups then touch one contiguous piece of the table -- 1 / nBins
 * of it -- and the workgroups of one XCD take one bin at a time, so the piece is read from that XCD's L2; every element
 * becomes (ordinal << 32 | index) in place; and because the scatter kernel noted where each sub-chunk's run of every bin
 * went (runTab), a workgroup per sub-chunk pulls its 16384 ordinals' results back from the nBins runs into an LDS tile and
 * writes them out in order: no second sort, no random store.  Semantics: modsetIndexFind (ms, kmer, false), modset.c:45-62. */
__global__ __launch_bounds__ (256)
void mgBinFindKernel (const MgSlot *__restrict__ slots, MgGeom g, MgPartFmt f, U64 *__restrict__ el, const U64 *__restrict__ binStart,
                      U32 nBins, U32 wgPerXcd)
{
  const U32 xcd = blockIdx.x & 7, j = blockIdx.x >> 3;      /* workgroups b, b + 8, ... share an XCD (observed placement; speed only) */
  const U64 ordMask = ((U64) 1 << f.ordBits) - 1;
  for (U32 b = xcd ; b < nBins ; b += 8)
    { const U64 lo = binStart[b], hi = binStart[b + 1];
      for (U64 i = lo + (U64) j * 256 + threadIdx.x ; i < hi ; i += (U64) wgPerXcd * 256)      /* (four lookups in flight per thread: 3.4 against 2.8 ms) */
        { const U64 x = __builtin_nontemporal_load (&el[i]);
          const U64 m = ((U64) b << f.remBits) | (x >> f.ordBits), key = m + 1;
          const U64 base = (U64) mgBucketOfM (m, g) * g.R;
          const U32 res = mgProbeFind (MgTableSlots { slots + base }, mgHomeOfM (m, g), g.R, key);
          __builtin_nontemporal_store (((x & ordMask) << 32) | res, &el[i]);
        }
    }
}

/* One tile of a pull-back, the whole workgroup (1024 threads): runRow[b] = where the tile's run of bin b went and its length (what the
 * scatter kernel noted); 16 waves take the runs in turn, 64 elements at a time, and dec (place in the partitioned array, &pos, &val)
 * says which place of the tile an element's result belongs to and what it is; then the tile's cnt results leave in order
 * (NT: non-temporal stores). */
template <int SUB, bool NT, class Decode>
__device__ __forceinline__ void mgPullTile (const unsigned long long *__restrict__ runRow, U32 nBins, const Decode &dec, U32 cnt, U32 *__restrict__ out)
{
  __shared__ U32 sTile[SUB];
  __shared__ unsigned long long sRun[MG_PART_MAXBINS];
  const U32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (U32 b = tid ; b < nBins ; b += 1024) sRun[b] = runRow[b];
  __syncthreads ();
  for (U32 b = wave ; b < nBins ; b += 16)
    { const unsigned long long r = sRun[b];
      const U64 base = r & (((U64) 1 << 40) - 1); const U32 len = (U32) (r >> 40);
      for (U32 i = lane ; i < len ; i += 64) { U32 pos, val; dec (base + i, &pos, &val); sTile[pos] = val; }
    }
  __syncthreads ();
  for (U32 i = tid ; i < cnt ; i += 1024) { if (NT) __builtin_nontemporal_store (sTile[i], &out[i]); else out[i] = sTile[i]; }
  __syncthreads ();
}

/* one level: every element is (ordinal << 32 | index) by now; a workgroup per sub-chunk of ordinals */
template <int SUB>
__global__ __launch_bounds__ (1024)
void mgUnpartKernel (const U64 *__restrict__ el, const unsigned long long *__restrict__ runTab, U32 nBins, U64 n, U32 *__restrict__ out)
{
  const U64 nSub = (n + SUB - 1) / SUB;
  for (U64 s = blockIdx.x ; s < nSub ; s += gridDim.x)
    { const U64 o0 = s * SUB;
      const auto dec = [=] (U64 at, U32 *pos, U32 *val) { const U64 v = __builtin_nontemporal_load (&el[at]); *pos = (U32) ((v >> 32) - o0); *val = (U32) v; };
      mgPullTile<SUB, true> (runTab + s * nBins, nBins, dec, (U32) (o0 + SUB < n ? SUB : n - o0), out + o0);
    }
}

/* ---- two levels (MODGPU_FIND_PATH=2): the second partition pass of the build as well, so that a bucket's lookups are contiguous
 * and the bucket (64 KiB) sits in LDS while they run.  The second pass replaces every element's ordinal by its position in the
 * first pass's output, where the element itself (with its ordinal) stays; results come back in two pulls: (chunk, half) tiles of
 * the first pass's output from the second pass's runs, then sub-chunks of ordinals from the first pass's runs. ---- */
/* WORD8: out of the 8-byte-per-slot copy of the table (find8, made by mgTablePack8Kernel below) instead of the table's own slots */
template <bool WORD8>
__global__ __launch_bounds__ (1024)
void mgBucketFindKernel (const MgSlot *__restrict__ slots, const U64 *__restrict__ find8, const U32 *__restrict__ occ, MgGeom g, MgPartFmt f, U32 nBuckets, int remB,
                         const U64 *__restrict__ bucketStart, U64 *__restrict__ el, U32 bucketsPerBlock)
{
  const U32 R = g.R, T = blockDim.x, tid = threadIdx.x;
  unsigned long long *sKey = reinterpret_cast<unsigned long long *> (mgDynLds);      /* WORD8: the copy's words, and no sIdx */
  U32 *sIdx = reinterpret_cast<U32 *> (mgDynLds + (size_t) R * 8);
  const U64 posMask = ((U64) 1 << f.ordBits) - 1, remMask = ((U64) 1 << remB) - 1;
  U32 b = blockIdx.x * bucketsPerBlock, bEnd = b + bucketsPerBlock;
  if (bEnd > nBuckets) bEnd = nBuckets;
  for ( ; b < bEnd ; ++b)
    { const U64 lo = bucketStart[b], hi = bucketStart[b + 1];
      if (hi == lo) continue;                                /* (uniform) */
      const bool any = occ[b] != 0;
      if (any)
        { for (U32 i = tid ; i < R ; i += T)
            if (WORD8) sKey[i] = __builtin_nontemporal_load (&find8[(U64) b * R + i]);
            else
              { const uint4 v = *reinterpret_cast<const uint4 *> (&slots[(U64) b * R + i]);
                sKey[i] = mgKeyOf (v); sIdx[i] = mgIndexOf (v.z);
              }
          __syncthreads ();
        }
      for (U64 i = lo + tid ; i < hi ; i += T)
        { const U64 x = __builtin_nontemporal_load (&el[i]);
          U32 res = 0;
          if (any)
            { const U64 m = ((U64) (b >> f.loB) << f.remBits) | (x >> f.ordBits);
              res = WORD8 ? mgProbeFind (MgImageWords8 { sKey }, mgHomeOfM (m, g), R, (m & remMask) + 1)
                          : mgProbeFind (MgImageSlots { sKey, sIdx }, mgHomeOfM (m, g), R, m + 1);
            }
          __builtin_nontemporal_store (((x & posMask) << 32) | res, &el[i]);
        }
      __syncthreads ();                                      /* the image is loaded again for the next bucket */
    }
}

/* The 8-byte-per-slot copy of the table (round 6).  The two-level lookups STREAM the table once per batch -- 16 bytes a slot of which
 * a lookup needs the key and the index; a bucket implies the key's leading bits, so where 2k - log2 NB <= 32 both fit one word:
 * (key's bits below the bucket id + 1) << 31 | index (0: the key has none), 0 = empty.  The copy (MgTable.find8) is made by mgTablePack8Kernel when a lookup batch finds
 * it missing or older than the table (one streaming pass), and a batch then reads half the bytes: config 3's table 1.9 -> 0.95 GB per batch. */
__global__ __launch_bounds__ (256)
void mgTablePack8Kernel (const MgSlot *__restrict__ slots, const U32 *__restrict__ occ, U32 nBuckets, U32 R, int remB, U64 *__restrict__ out)
{
  const U64 remMask = ((U64) 1 << remB) - 1;
  for (U32 b = blockIdx.x ; b < nBuckets ; b += gridDim.x)
    { if (!occ[b]) continue;                                /* (never read: the lookups ask occ[] first) */
      for (U32 i = threadIdx.x ; i < R ; i += blockDim.x)
        { const uint4 v = *reinterpret_cast<const uint4 *> (&slots[(U64) b * R + i]);
          const U64 key = mgKeyOf (v);
          U64 w = 0;            /* a keyed slot without an index (an add that was refused left it) keeps its key and answers 0: the chain goes on, as in the 16-byte table */
          if (key) w = ((((key - 1) & remMask) + 1) << 31) | (U64) mgIndexOf (v.z);
          __builtin_nontemporal_store (w, &out[(U64) b * R + i]);
        }
    }
}

/* the second level's results back into the order of the first pass's output: a workgroup per (chunk, half) of that output */
template <int SUB>
__global__ __launch_bounds__ (1024)
void mgUnpartPosKernel (const U64 *__restrict__ el, const unsigned long long *__restrict__ runTab, U32 nBins,
                        const U64 *__restrict__ segStart, const U32 *__restrict__ chunkBase, U32 nSeg, U32 chunkElems, U32 *__restrict__ idxOut)
{
  const U32 nChunks = chunkBase[nSeg];
  for (U32 w = blockIdx.x ; w < 2 * nChunks ; w += gridDim.x)
    { const U32 c = w >> 1, h = w & 1;
      U32 seg; U64 lo, hi;
      if (!mgChunkRange (segStart, chunkBase, nSeg, chunkElems, c, &seg, &lo, &hi)) continue;
      const U64 sub = lo + (U64) h * SUB;
      if (sub >= hi) continue;                               /* (uniform) */
      const auto dec = [=] (U64 at, U32 *pos, U32 *val) { const U64 v = __builtin_nontemporal_load (&el[at]); *pos = (U32) ((v >> 32) - sub); *val = (U32) v; };
      mgPullTile<SUB, false> (runTab + (U64) w * nBins, nBins, dec, (U32) (sub + SUB < hi ? SUB : hi - sub), idxOut + sub);
    }
}

/* the first level's pull when the results sit beside the elements (idx[]) and the elements still hold their ordinals */
template <int SUB>
__global__ __launch_bounds__ (1024)
void mgUnpartOrdKernel (const U64 *__restrict__ el, const U32 *__restrict__ idx, int ordBits, const unsigned long long *__restrict__ runTab, U32 nBins, U64 n,
                        U32 *__restrict__ out)
{
  const U64 nSub = (n + SUB - 1) / SUB, ordMask = ((U64) 1 << ordBits) - 1;
  for (U64 s = blockIdx.x ; s < nSub ; s += gridDim.x)
    { const U64 o0 = s * SUB;
      const auto dec = [=] (U64 at, U32 *pos, U32 *val) { *pos = (U32) ((__builtin_nontemporal_load (&el[at]) & ordMask) - o0); *val = __builtin_nontemporal_load (&idx[at]); };
      mgPullTile<SUB, true> (runTab + s * nBins, nBins, dec, (U32) (o0 + SUB < n ? SUB : n - o0), out + o0);
    }
}

/* ======================================================================================== */
/* host side                                                                                  */

MgStatus mgTableFind (MgTable *t, const U64 *dKmer, U64 n, U32 *dIndexOut, hipStream_t st)
{
  if (!n) return MG_OK;
  /* with the never-written buckets zeroed once, a probe needs no look at occ[] first */
  { MgStatus cs = mgTableClean (t, st); if (cs) return cs; }
  const unsigned fgrid = mgGridWide ((n + MG_FIND_PER - 1) / MG_FIND_PER);
  ++t->diag[MG_DIAG_FIND_DIRECT];
  MG_LAUNCH (MG_K_TABLE_FIND, st, mgTableFindKernel<false>, dim3 (fgrid), dim3 (256), 0, st, t->slots, t->occ, mgGeomOf (t), dKmer, n, dIndexOut);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

MgStatus mgTableFindSegments (MgTable *t, const MgSegSrc &src, U64 n, U32 *dIndexOut, hipStream_t st)
{
  if (!n) return MG_OK;
  { MgStatus cs = mgTableClean (t, st); if (cs) return cs; }
  const U64 nRows = (n + 63) / 64;
  U64 waves = 256ull * 4 * 8;                           /* eight waves per SIMD */
  if (waves > nRows) waves = nRows;
  const U64 rowsPerWave = (nRows + waves - 1) / waves;
  waves = (nRows + rowsPerWave - 1) / rowsPerWave;
  ++t->diag[MG_DIAG_FIND_DIRECT];
  MG_LAUNCH (MG_K_TABLE_FIND_SEG, st, mgTableFindSegKernel, dim3 ((unsigned) ((waves + 3) / 4)), dim3 (256), 0, st, t->slots, mgGeomOf (t), src, n, rowsPerWave, dIndexOut);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

/* does a lookup batch take the partitioned path?  It needs the scan's digit counts for this table geometry, elements that
   fit one word, and a table the direct probes would have to fetch from HBM */
/* The digit of the partitioned lookup: the top bits of the bucket id one pass sorts by; a bin's piece of the table is
   nSlots * 16 bytes >> bits (MODGPU_FIND_BITS: dev, 3..9) */
int mgTableFindDigitBits (const MgTable *t)
{
  const long kb = mgKnobs ()->findBits;
  int hiB, loB; mgPartSplit (t->log2NB, &hiB, &loB);          /* the build's own first digit: 256 bins of 8 MB at config 3 (512 bins of 4 MB: scatter and pull-back cost 0.7 ms more, the lookups gain nothing) */
  int bits = kb != MG_KNOB_UNSET && kb >= 3 && kb <= 9 ? (int) kb : hiB;
  if (bits > t->log2NB) bits = t->log2NB;
  return bits;
}

bool mgTableFindTakesPartition (const MgTable *t, U64 n, const MgHistReq *counted)
{
  const long kp = mgKnobs ()->findPath;                      /* test knob: 'p' / 'd' force it */
  if (kp == 'd') return false;
  if (!n || !counted || !counted->binCount || counted->log2NB != t->log2NB || counted->kbits != t->kbits) return false;
  const int hiB = counted->hiB;
  if (hiB != mgTableFindDigitBits (t)) return false;
  if (!mgPartFmtFits (t, mgPartFmtOf (t, n, hiB)) || hiB < 3) return false;
  if (t->kbits < 24 || mgKnobs ()->scanHist == 0) return false;          /* (the counts must be the scan's own: mgLaunchScanRange) */
  if (kp == 'p' || kp == '2') return true;
  /* by itself: the two-level path where the direct probes would fetch a line from HBM per lookup -- a table of 256 MB and more,
     a batch that fills the chip (config 3: 3.5 against 4.2-4.6 ms per 1.56e8 lookups; one level ties with the direct probes) */
  return n >= ((U64) 1 << 24) && t->nSlots >= ((U64) 1 << 24) && t->log2NB > 9;
}

/* scratch of the partitioned lookup for a batch of n: the run table and the partition's small arrays (the packed elements,
   8 bytes each, go where the caller says: the scan's unused dense k-mer array) */
size_t mgTableFindPartScratchBytes (U64 n)
{
  return mgAl256 ((n / MG_PART_SUB + 2) * (size_t) MG_PART_MAXBINS * 8) + mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8) * 2
       + mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8 * 16) + mgAl256 ((MG_PART_MAXBINS + 2) * 4)
       + mgAl256 ((MG_PART_MAXBINS + 2 + n / MG_PART_CHUNK + MG_PART_MAXBINS + 2) * 4) + mgAl256 ((n / MG_PART_SUB + 2) * sizeof (MgSubSeg)) + 4096;
}

/* the two-level path's extra scratch: the second pass's output (8 bytes an element), the results beside the first pass's output
   (4), the second run table, the fine starts / cursors / counts and its chunk table */
size_t mgTableFindPart2ScratchBytes (U64 n)
{
  const U64 NB = (U64) 1 << 18;
  return mgAl256 (n * 8) + mgAl256 (n * 4) + mgAl256 ((2 * (n / (2 * (U64) MG_PART_SUB) + MG_PART_MAXBINS + 2)) * (size_t) MG_PART_MAXBINS * 8)
       + mgAl256 ((NB + 2) * 8) + mgAl256 ((NB + 2 + (U64) MG_PART_MAXBINS * 16) * 8) + mgAl256 ((NB + 2) * 4)
       + mgAl256 ((MG_PART_MAXBINS + 2 + n / MG_PART_CHUNK + MG_PART_MAXBINS + 2) * 4) + 4096;
}

MgStatus mgTableFindPartitioned (MgTable *t, const MgSegSrc &segSrc, U64 n, const MgHistReq *counted, U32 *dIndexOut, U64 *el, void *scratch, hipStream_t st,
                                 void *scratch2)
{
  if (!n) return MG_OK;
  { MgStatus cs = mgTableClean (t, st); if (cs) return cs; }
  char *wb = (char *) scratch;
  unsigned long long *runTab = (unsigned long long *) wb;    wb += mgAl256 ((n / MG_PART_SUB + 2) * (size_t) MG_PART_MAXBINS * 8);
  U64 *binStart = (U64 *) wb;                                wb += mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8);
  U64 *whole = (U64 *) wb;                                   wb += mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8);
  unsigned long long *cursor = (unsigned long long *) wb;    wb += mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8 * 16);
  U32 *binCount = (U32 *) wb;                                wb += mgAl256 ((MG_PART_MAXBINS + 2) * 4);
  U32 *chunkBase = (U32 *) wb;                               wb += mgAl256 ((MG_PART_MAXBINS + 2 + n / MG_PART_CHUNK + MG_PART_MAXBINS + 2) * 4);
  MgSubSeg *subSeg = (MgSubSeg *) wb;                        wb += mgAl256 ((n / MG_PART_SUB + 2) * sizeof (MgSubSeg));
  const int hiB = counted->hiB, loB = t->log2NB - hiB;
  const MgPartFmt f = mgPartFmtOf (t, n, hiB);
  const U32 nBins = (U32) 1 << hiB;
  U64 segInit[2] = { 0, n };
  MG_HIP (hipMemcpyAsync (whole, segInit, 16, hipMemcpyHostToDevice, st));
  const bool twoLevels = scratch2 && loB > 0 && ((U32) 1 << loB) <= MG_PART_MAXBINS;
  /* (two levels) the fine digits as bytes beside the first pass's output, for the second pass's counts: in idxA, which is only written by the first pull */
  unsigned char *digits = (twoLevels && loB <= 8 && mgKnobs ()->partDigits != 0) ? reinterpret_cast<unsigned char *> ((char *) scratch2 + mgAl256 (n * 8)) : 0;
  MgPartPassArgs p1 = {};                /* the build's first pass: from the scan's segments and its counts into el, by the coarse digit; runTab says where every sub-chunk went */
  p1.inMode = MG_EL_SEG; p1.packed = true; p1.f = f; p1.n = n; p1.segStart = whole; p1.nSeg = 1; p1.shift = loB; p1.nBins = nBins;
  p1.kOut = el; p1.binStart = binStart; p1.cursor = cursor; p1.binCount = binCount; p1.chunkBase = chunkBase;
  p1.counted = counted->binCount; p1.segSrc = &segSrc; p1.subSeg = subSeg; p1.runTab = runTab; p1.digitOut = digits; p1.nextBins = (U32) 1 << loB;
  MgStatus s = mgPartPass (t, p1, st);
  if (s) return s;
  const U32 subElems = p1.subElems;
  if (twoLevels)      /* ---- two levels: the lookups bucket by bucket out of LDS (a table of few buckets has no fine digit: one level) ---- */
    { char *w2 = (char *) scratch2;
      const U64 NB = (U64) 1 << t->log2NB;
      U64 *el2 = (U64 *) w2;                                   w2 += mgAl256 (n * 8);
      U32 *idxA = (U32 *) w2;                                  w2 += mgAl256 (n * 4);
      unsigned long long *runTab2 = (unsigned long long *) w2; w2 += mgAl256 ((2 * (n / (2 * (U64) MG_PART_SUB) + MG_PART_MAXBINS + 2)) * (size_t) MG_PART_MAXBINS * 8);
      U64 *fineStart = (U64 *) w2;                             w2 += mgAl256 ((NB + 2) * 8);
      unsigned long long *fineCursor = (unsigned long long *) w2; w2 += mgAl256 ((NB + 2 + (U64) MG_PART_MAXBINS * 16) * 8);
      U32 *fineCount = (U32 *) w2;                             w2 += mgAl256 ((NB + 2) * 4);
      U32 *chunkBase2 = (U32 *) w2;                            w2 += mgAl256 ((MG_PART_MAXBINS + 2 + n / MG_PART_CHUNK + MG_PART_MAXBINS + 2) * 4);
      const U32 nBins2 = (U32) 1 << loB;
      MgPartPassArgs p2 = {};            /* the second pass: el's bins by the fine digit into el2, every element's ordinal replaced by its place in el (runMode 1) */
      p2.inMode = MG_EL_PACKED; p2.packed = true; p2.f = f; p2.kIn = el; p2.n = n; p2.segStart = binStart; p2.nSeg = nBins; p2.nBins = nBins2;
      p2.kOut = el2; p2.binStart = fineStart; p2.cursor = fineCursor; p2.binCount = fineCount; p2.chunkBase = chunkBase2;
      p2.runTab = runTab2; p2.runMode = 1; p2.digitIn = digits;
      if ((s = mgPartPass (t, p2, st))) return s;
      const U32 sub2 = p2.subElems;
      U32 perBlock;
      const unsigned bGrid = mgBucketGrid (NB, &perBlock);
      const int remB = t->kbits - t->log2NB;
      const bool word8 = remB >= 1 && remB <= 32 && mgKnobs ()->find8 != 0;          /* (rem + 1 <= 2^32 above a 31-bit index: one word) */       /* (test knob MODGPU_FIND8=0: the 16-byte table itself) */
      if (word8 && (!t->find8 || t->find8Version != t->version || t->find8Cap < t->nSlots))
        { if (t->find8Cap < t->nSlots)
            { if (t->find8) { MG_HIP (hipStreamSynchronize (st)); MG_HIP (hipFree (t->find8)); t->find8 = 0; t->find8Cap = 0; }
              MG_HIP (hipMalloc ((void **) &t->find8, t->nSlots * sizeof (U64)));
              t->find8Cap = t->nSlots;
            }
          ++t->diag[MG_DIAG_PACK8];
          MG_LAUNCH (MG_K_TABLE_LOAD, st, mgTablePack8Kernel, dim3 ((unsigned) (NB < 8192 ? NB : 8192)), dim3 (256), 0, st, t->slots, t->occ, (U32) NB, t->R, remB, t->find8);
          t->find8Version = t->version;
        }
      const size_t lds = (size_t) t->R * (word8 ? 8 : 12) + 16;
      s = mgForFlag (word8, [&] (auto W8) -> MgStatus
        { if (lds > 48 * 1024) MG_HIP (hipFuncSetAttribute ((const void *) mgBucketFindKernel<decltype (W8)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
          ++t->diag[word8 ? MG_DIAG_FIND_PART2_8 : MG_DIAG_FIND_PART2_16];
          MG_LAUNCH (MG_K_BUCKET_FIND, st, mgBucketFindKernel<decltype (W8)::value>, dim3 (bGrid), dim3 (1024), lds, st,
                     t->slots, word8 ? t->find8 : (const U64 *) 0, t->occ, mgGeomOf (t), f, (U32) NB, word8 ? remB : 0, fineStart, el2, perBlock);
          return MG_OK;
        });
      if (s) return s;
      const unsigned g2 = 2 * p2.maxChunks < 2048 ? 2 * p2.maxChunks : 2048;
      mgForSub (sub2, [&] (auto S) { MG_LAUNCH (MG_K_UNPART, st, mgUnpartPosKernel<decltype (S)::value>, dim3 (g2), dim3 (1024), 0, st, el2, runTab2, nBins2, binStart, chunkBase2, nBins, 2 * sub2, idxA); });
      const U64 nSub1 = (n + subElems - 1) / subElems;
      const unsigned g1 = (unsigned) (nSub1 < 2048 ? nSub1 : 2048);
      mgForSub (subElems, [&] (auto S) { MG_LAUNCH (MG_K_UNPART, st, mgUnpartOrdKernel<decltype (S)::value>, dim3 (g1), dim3 (1024), 0, st, el, idxA, f.ordBits, runTab, nBins, n, dIndexOut); });
      MG_HIP (hipGetLastError ());
      return MG_OK;
    }
  const U32 wgPerXcd = 256;                                  /* 2048 workgroups of 256: eight waves per SIMD */
  ++t->diag[MG_DIAG_FIND_PART1];
  MG_LAUNCH (MG_K_BUCKET_FIND, st, mgBinFindKernel, dim3 (8 * wgPerXcd), dim3 (256), 0, st, t->slots, mgGeomOf (t), f, el, binStart, nBins, wgPerXcd);
  const U64 nSub = (n + subElems - 1) / subElems;
  const unsigned ug = (unsigned) (nSub < 2048 ? nSub : 2048);
  mgForSub (subElems, [&] (auto S) { MG_LAUNCH (MG_K_UNPART, st, mgUnpartKernel<decltype (S)::value>, dim3 (ug), dim3 (1024), 0, st, el, runTab, nBins, n, dIndexOut); });
  MG_HIP (hipGetLastError ());
  return MG_OK;
}
