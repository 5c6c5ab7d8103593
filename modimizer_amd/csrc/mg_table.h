/* mg_table.h — what the files of the device modset table share: mg_table.hip (layout, life cycle), mg_tableadd.hip (mgTableAdd: direct
 * build, plan, scratch, launches), mg_rank.hip (ordered flag count), mg_tableset.hip (whole-set passes), mg_part.hip (radix partition),
 * mg_bucket.hip (one workgroup per bucket: dedup, merge, rank lookups) and mg_find.hip (lookups).
 * Internal to those seven; the library's interface to the table is in mg_common.h.
 *
 * One file per kernel: a kernel or kernel template is defined in exactly one .hip file, and every launch of it and every
 * hipFuncSetAttribute on it is in that file.  This header holds no kernel and nothing that instantiates one -- otherwise two objects
 * would carry copies of an instance, and an attribute set on one copy would not apply to the copy that launches. */
#ifndef MG_TABLE_H
#define MG_TABLE_H
#include <stdlib.h>
#include <string.h>
#include "mg_prefix.h"

#define MG_ASSIGNED 0x80000000u
#define MG_R_QUANTUM 64u              /* slots per bucket come in multiples of this (a bucket starts on a 1 KiB boundary) */
/* -DMG_BUILD_PRIO: the build's kernels raise their waves' issue priority (s_setprio 3).  An experiment of round 3 for running
 * them beside the instruction-bound scan of the next batch on a second stream ("scan || build"): with it the
 * co-run gains 9 % over no priority, but it still takes 93 % of the sum of the two (the build's kernels need the wave slots the
 * scan holds), and alone the partition scatter loses 9 % and the merge 5 % to it -- so it is off. */
#ifdef MG_BUILD_PRIO
#define MG_BUILD_PRIO() __builtin_amdgcn_s_setprio (3)
#else
#define MG_BUILD_PRIO() do { } while (0)
#endif
#ifdef MG_ABLATE
#define MG_ABLATE_AND(x) && (x)
#else
#define MG_ABLATE_AND(x)
#endif
__device__ __forceinline__ U32 mgToken (U64 o) { return 0x7fffffffu - (U32) o; }     /* 1..0x7fffffff */
__device__ __forceinline__ bool mgIsAssigned (U32 v) { return (v & MG_ASSIGNED) != 0; }
/* a 16-byte slot read as one uint4 {key lo, key hi, ord, cnt}: its key, the index its ordinal word holds (0: none yet), and
   "an entry with an index up to keepMax" -- what a rehash keeps */
__device__ __forceinline__ U64 mgKeyOf (const uint4 &v) { return ((U64) v.y << 32) | v.x; }
__device__ __forceinline__ U32 mgIndexOf (U32 ordWord) { return mgIsAssigned (ordWord) ? (ordWord & ~MG_ASSIGNED) : 0; }
__device__ __forceinline__ bool mgLiveEntry (const uint4 &v, U32 keepMax) { return (v.x | v.y) && mgIsAssigned (v.z) && (v.z & ~MG_ASSIGNED) <= keepMax; }

/* bucket geometry: MgGeom, mgMixK, mgBucketOfM, mgHomeOfM in mg_common.h */

/* counters[]: 0 = new entries this call, 1 = bucket overflow flag */

/* the rank record mgRankRecordKernel (mgTablePrune: mgRankAssignKernel; both mg_rank.hip) leaves per row of 64 ordinals: the row's flags and the number of flags before it */
struct __attribute__ ((aligned (16))) MgRankGrp { U64 bits; U32 rank; U32 pad; };   /* per 64 ordinals */

/* ---- k-mers read from the scan's segments (MgSegSrc) instead of a dense array ---------------------------------
 * A wave reads 64 consecutive ordinals at a time; they lie in one segment, rarely in two or more.  The wave keeps the
 * segment of its first ordinal in scalar registers (w, its first ordinal s0 and the next segment's s1) and walks it
 * forward as its ordinals grow; a lane behind s1 walks on by itself. */
#ifndef MG_PART_SUB
#define MG_PART_SUB 8192
#endif                            /* elements of a sub-chunk of the partition passes (LDS counting sort) */
struct MgSegCursor { U32 w; U64 s0, s1; };
__device__ __forceinline__ U64 mgUniform64 (U64 x)
{ return ((U64) (U32) __builtin_amdgcn_readfirstlane ((int) (U32) (x >> 32)) << 32) | (U32) __builtin_amdgcn_readfirstlane ((int) (U32) x); }
/* the segment holding ordinal o (o < total): first w with segStart[w + 1] > o */
__device__ __forceinline__ U32 mgSegOfOrdinal (const MgSegSrc &src, U64 o)
{
  U32 a = 0, b = src.nSegs - 1;
  while (a < b) { const U32 m = (a + b) / 2; if (src.segStart[m + 1] > o) b = m; else a = m + 1; }
  return a;
}
/* (w and o0 are the same in every lane: saying so keeps the cursor and its loads on the scalar unit) */
__device__ __forceinline__ void mgSegCursorAt (const MgSegSrc &src, U32 w, MgSegCursor *c)
{ w = (U32) __builtin_amdgcn_readfirstlane ((int) w); c->w = w; c->s0 = mgUniform64 (src.segStart[w]); c->s1 = mgUniform64 (src.segStart[w + 1]); }
/* advance to the segment of o0 (uniform, o0 < total, not before the cursor) */
__device__ __forceinline__ void mgSegCursorSeek (const MgSegSrc &src, MgSegCursor *c, U64 o0)
{ o0 = mgUniform64 (o0); while (c->s1 <= o0) { ++c->w; c->s0 = c->s1; c->s1 = mgUniform64 (src.segStart[c->w + 1]); } }
/* address of this lane's ordinal i = o0 + lane, for a cursor at o0 (uniform) and `last` = the last ordinal any lane asks
 * for (uniform, < total).  The walk over the segments the 64 ordinals touch is the same in every lane and loads through
 * the scalar unit only: a vector load inside it would make the compiler drain the k-mer loads already in flight. */
__device__ __forceinline__ const U64 *mgSegAddr (const MgSegSrc &src, const MgSegCursor &c, U64 i, U64 last)
{
  U32 w = c.w; U64 b0 = c.s0, b1 = c.s1;
  const U64 *addr = src.segKmer + (U64) w * src.segCap + (i - b0);
  last = mgUniform64 (last);
  while (b1 <= last)
    { ++w; b0 = b1; b1 = mgUniform64 (src.segStart[w + 1]);
      if (i >= b0) addr = src.segKmer + (U64) w * src.segCap + (i - b0);
    }
  return addr;
}

/* subSeg[q] = the cursor at ordinal q * MG_PART_SUB (w, s0, s1): where the first partition pass starts a sub-chunk's
 * walk and the index assignment a wave's (one load instead of a binary search of dependent ones) */
struct __attribute__ ((aligned (8))) MgSubSeg { U64 w, s0, s1; };
__device__ __forceinline__ void mgSegCursorFrom (const MgSubSeg *__restrict__ subSeg, U64 q, MgSegCursor *c)
{ const MgSubSeg e = subSeg[q]; c->w = (U32) __builtin_amdgcn_readfirstlane ((int) (U32) e.w); c->s0 = mgUniform64 (e.s0); c->s1 = mgUniform64 (e.s1); }

/* ---- the radix partition (mg_part.hip) ---- */
#define MG_PART_CHUNK (2 * MG_PART_SUB)          /* elements per workgroup pass, at least (a pass with larger sub-chunks takes two of those) */
#define MG_PART_MAXBINS 512

/* What a partition pass reads and writes.  The first pass reads the dense k-mers (an element's ordinal is its
 * position) and mixes them; from then on everything is in mixed space.  Two element formats:
 *   wide    8 bytes of mixed k-mer + 4 bytes of ordinal (separate arrays): any k, any batch size;
 *   packed  one 8-byte word (rem << ordBits) | ordinal, where rem = the mixed k-mer WITHOUT its coarse digit (the
 *           bin the element sits in implies those hiB bits: the mix is a bijection and the bucket id is a prefix of
 *           it) and ordBits = bits of the batch's largest ordinal.  Fits when 2k - hiB + ordBits <= 64, e.g. k = 21
 *           with 2^28 modimizers: 34 + 28 bits.  A third less traffic in both passes and in the dedup kernel. */
#define MG_EL_DENSE  0      /* input of the first pass: k-mers, ordinal = index */
#define MG_EL_WIDE   1      /* (mixed k-mer, ordinal) */
#define MG_EL_PACKED 2      /* (rem << ordBits) | ordinal */
#define MG_EL_SEG    3      /* input of the first pass when the k-mers still sit in the scan's segments (MgSegSrc): ordinal = position in the concatenation */
struct MgPartFmt { int ordBits, remBits, loB; };      /* remBits = 2k - hiB; loB = bits of the fine digit */

/* digit of an element = bits [shift, shift+log2(nBins)) of its bucket id */
template <int MODE>
__device__ __forceinline__ U32 mgDigitOf (U64 x, const MgGeom &g, const MgPartFmt &f, int shift, U32 binMask)
{
  if (MODE == MG_EL_DENSE)  return (mgBucketOfM (mgMixK (x, g.kbits), g) >> shift) & binMask;
  if (MODE == MG_EL_WIDE)   return (mgBucketOfM (x, g) >> shift) & binMask;
  return (U32) (x >> (f.ordBits + f.remBits - f.loB)) & binMask;      /* packed: only ever asked for the fine digit, the top loB bits of rem */
}

/* chunk -> (segment, range): segments are [segStart[s], segStart[s+1]); chunkBase[s] = first chunk of s,
 * chunkBase[nSeg] = number of chunks, and behind that table (at MG_CHUNK_SEG_AT) the segment of every chunk, so
 * that a workgroup moving to its next chunk does two rounds of loads, not a binary search of dependent ones */
#define MG_CHUNK_SEG_AT (MG_PART_MAXBINS + 2)
__device__ __forceinline__ bool mgChunkRange (const U64 *__restrict__ segStart, const U32 *__restrict__ chunkBase, U32 nSeg, U32 chunkElems,
                                              U32 chunk, U32 *seg, U64 *lo, U64 *hi)
{
  if (chunk >= chunkBase[nSeg]) return false;
  const U32 a = chunkBase[MG_CHUNK_SEG_AT + chunk];
  *seg = a;
  *lo = segStart[a] + (U64) (chunk - chunkBase[a]) * chunkElems;
  U64 e = segStart[a + 1];
  *hi = *lo + chunkElems < e ? *lo + chunkElems : e;
  return true;
}

#ifndef MG_PART_THREADS
#define MG_PART_THREADS 1024
#endif
/* Sub-chunks of MG_PART_SUB_BIG elements where they fit the LDS -- one packed 8-byte word per element, at most 256 bins, so that a staged
 * element's digit is one byte: 152 KB.  A bin's run is then 64 elements (512 bytes) instead of 32, and the barriers, the scan of the
 * counts and the reservations are paid once per 16384 elements: the two passes 1.335 -> 1.235 ms at config 2. */
#define MG_PART_SUB_BIG (2 * MG_PART_SUB)
#define MG_PART_BIG_BINS 256

/* One partition pass: nSeg segments of kIn -> nBins bins each.  What is not set stays 0: not there, not wanted. */
struct MgPartPassArgs {
  int inMode; bool packed; MgPartFmt f;            /* inMode: what kIn holds (MG_EL_*); packed: the format of the output (and, after the first pass, of the input) */
  const U64 *kIn; const U32 *tIn; U64 n;           /* the elements (tIn: the ordinals of wide ones) */
  const U64 *segStart; U32 nSeg;                   /* [nSeg + 1] the segments of kIn */
  int shift; U32 nBins;                            /* the digit: bits [shift, shift + log2 nBins) of the bucket id */
  U64 *kOut; U32 *tOut; U64 *binStart;             /* out: the elements by (segment, bin), and [nSeg x nBins + 1] where every bin starts */
  unsigned long long *cursor; U32 *binCount, *chunkBase;   /* work space */
  const U32 *counted;                              /* the digit counts the scan made (one segment), instead of a counting pass */
  const MgSegSrc *segSrc; MgSubSeg *subSeg;        /* MG_EL_SEG: the scan's segments the k-mers sit in (with counted), and work space */
  unsigned long long *runTab; int runMode;         /* the partitioned lookup: out, where every sub-chunk's run of every bin went (mgPartScatterKernel) */
  unsigned char *digitOut; int nextShift; U32 nextBins;    /* out: the NEXT pass's digit (bits [nextShift, ..) of the bucket id, nextBins <= 256 of them) of every element, beside it */
  const unsigned char *digitIn;                    /* such bytes of the pass before: the digits are counted from them */
  U32 subElems, maxChunks;                         /* out: elements of a sub-chunk (a chunk is two), and a bound on the chunks */
};
MgStatus mgPartPass (const MgTable *t, MgPartPassArgs &p, hipStream_t st);

/* ---- one workgroup per bucket, the bucket in LDS (mg_bucket.hip; the lookups of mg_find.hip and the rehash of mg_table.hip too) ---- */
struct MgBucketArgs {
  MgSlot *slots; MgGeom g; U32 nBuckets;
  const U64 *bucketStart;          /* [NB+1] ranges into pK/pT/pC */
  U64 *pK; U32 *pT; U32 *pC;       /* in: occurrences, wide (mixed k-mer in pK, ordinal in pT) or packed (pK alone); out (in place over
                                      pK, and in pT / pC): uniques (mixed k-mer, ord field, count) */
  MgPartFmt f;                     /* packed format */
  U32 *uniqCount;                  /* [NB] */
  U32 *occ;                        /* [NB] entries per bucket */
  unsigned char *flags;            /* [n] first occurrence of a k-mer new to the table */
  const MgRankGrp *grp; U32 baseMax; U32 size;
  /* a bucket's uniques leave the dedup kernel grouped by the SLICE of the ordinal range their first occurrence lies in
     (groups 0..nSlices-1: new k-mers of slice tok >> sliceShift; group nSlices: k-mers the table already holds), so that
     the rank lookups can run slice by slice against a piece of the rank records that stays in the L2 */
  unsigned short *sliceOff;        /* [NB x (nSlices + 2)]: start of group g in bucket b's list; [nSlices + 1] = the list's length */
  U32 nSlices; int sliceShift;
  int slotShift;                   /* != 0 (2k <= 48): a list entry carries, above bit slotShift of its mixed k-mer, the slot the k-mer holds in
                                      the dedup kernel's LDS image of the bucket -- a valid place in the bucket (the image starts from the
                                      table's own), so the merge kernel puts it there without probing */
  int place;                       /* != 0: the merge kernel lays a bucket that was empty (occ = 0) out by prefix scan (mgPlaceFresh), without a probe */
  int markDup;                     /* which way round the flags are written: 0 = cleared by a memset, the dedup kernel sets the first occurrence
                                      of every new k-mer (one store per unique); 1 = preset to 1, it clears every occurrence that is NOT one (one
                                      store per duplicate: fewer when most of a batch's modimizers are new k-mers) */
  int withDepth;
  U64 *counters;
  /* oversize buckets (a k-mer with very many copies: poly-A, satellite monomers): a bucket of more than hotSplit occurrences is
     cut into chunks of mgHotChunkLen () occurrences, mgHotReduceKernel -- a workgroup per chunk -- reduces every chunk in place
     to weighted entries (one per distinct k-mer: its earliest ordinal in the chunk, its count in pC; pC = 0 ends a chunk's
     list), and the bucket's own workgroup in the dedup kernel walks the chunks' lists instead of the occurrences */
  U32 hotSplit, hotChunk;
  U64 *hotItems; unsigned long long *hotCount;     /* the chunks to reduce: (bucket << 32 | chunk), and how many ([0]; [1]: oversize buckets) */
  U32 *hotBuckets;                                 /* the oversize buckets, for the dedup kernel's HOT instance */
#ifdef MG_ABLATE
  int debug;                       /* ablation builds only (MODGPU_BUCKET_DEBUG): dedup: 1 no flag stores, 2 plain stores for max/add, 4 no claim loop, 8 no list stores; merge: 32 no claim loop, 64 no image stores; lookup: 16 no rank gathers, 128 no index stores, 256 no ordinal loads; the merge kernel's scan placement: 512 no home counts, 1024 no scans, 2048 no placement stores; results are wrong */
#endif
  unsigned long long *liveHist;    /* != 0: the merge kernel also counts the final depths of the entries it writes */
};

extern __shared__ __attribute__ ((aligned (16))) unsigned char mgDynLds[];

/* find-or-claim the LDS slot of key; returns R on overflow.  Linear probing: the slot is the first one of home, home + 1, ... (wrapping
 * inside the bucket) that holds the key or is empty.  This loop is what both bucket kernels spend their time in -- a workgroup waits at
 * its barrier for its LONGEST chain (8 links at load 0.38, 30 at 0.6, 80 at 0.75), every link a dependent LDS round trip -- and its code
 * shape counts (DESIGN_EXPERIMENTS.md section K: four slots a step, lanes walking independently, first probes issued together all made the
 * kernels slower).  The compare-and-swap IS the probe: one round trip where the slot is empty, not a read and then the swap (round 6:
 * dedup 1.32 -> 1.25 ms, merge 1.18 -> 1.07). */
__device__ __forceinline__ U32 mgLdsClaim (unsigned long long *sKey, U32 R, U32 home, unsigned long long key)
{
  U32 at = home;
  for (U32 probes = 0 ; probes < R ; ++probes)
    { const unsigned long long cur = atomicCAS (&sKey[at], 0ull, key);
      if (cur == 0 || cur == key) return at;
      at = mgNextSlot (at, R);
    }
  return R;
}

#ifndef MG_BUCKET_PREFETCH
#define MG_BUCKET_PREFETCH 3         /* occurrences per thread of the dedup kernel fetched one bucket ahead: with 1024 threads a whole bucket of config 2 (1.42 -> 1.20 ms against 2) */
#endif
#ifndef MG_MERGE_PREFETCH
#define MG_MERGE_PREFETCH 2          /* uniques per thread of the merge kernel fetched one bucket ahead */
#endif
#ifndef MG_HOT_DEPTH
#define MG_HOT_DEPTH 4                /* occurrences per thread and turn of the dedup kernel's loop over what was not fetched ahead */
#endif
#define MG_PLACE_KEEP 4              /* uniques per thread the merge kernel's scan placement takes: R <= 4 x threads, so every list of a bucket of up to 4096 slots */
#define MG_RANK_GROUPS 64            /* most groups a bucket's list is cut into: slices of the ordinal range + 1 */
#define MG_SLOT_SHIFT 48             /* a list entry's slot sits above this bit of its mixed k-mer (when 2k <= 48) */
#define MG_DEDUP_PER 4               /* slots of the LDS image per thread of the dedup kernel: R <= 4 x threads ... */
#define MG_DEDUP_PER_BIG 8           /* ... or 8 (R = 8192: a table of 2^31 slots, i.e. more than 6.4e8 entries at table bits 32; one workgroup per CU, 128 registers) */
#define MG_LIVE_BINS 256              /* depths below this are counted in LDS by the merge kernel's live histogram */
/* LDS of the merge kernel: the image (16 bytes a slot), 16 bytes, the live-depth bins, the scan's 2 x 16 words, start[] */
static inline size_t mgMergeLdsBytes (U32 R) { return (size_t) R * 16 + 16 + MG_LIVE_BINS * 4 + 128 + (size_t) R * 2; }

#define MG_HOT_SPLIT_DEFAULT 16384u  /* occurrences above which a bucket is reduced chunk by chunk first (a bucket of config 2 holds 2400); measured on the repeat-genome probe: 8192 / 16384 / 32768 / 65536 -> 1.50 / 1.44 / 1.48 / 1.50 ms per Gbp */
#define MG_HOT_CHUNK_DEFAULT 4096u   /* occurrences of a chunk, at least */
#define MG_HOT_MAXCHUNKS 1024u       /* chunks of a bucket, at most: a bucket of 1e9 occurrences is 1024 chunks of 1e6 */
__host__ __device__ __forceinline__ U64 mgHotChunkLen (U64 cnt, U32 minChunk)
{ const U64 L = (cnt + MG_HOT_MAXCHUNKS - 1) / MG_HOT_MAXCHUNKS; return L < minChunk ? minChunk : L; }
/* the launches of mgTableAdd's bucketed leg, in its order.  threads, grid, perBlock: mgBucketThreads, mgBucketGrid; lds: the launch's dynamic LDS */
MgStatus mgBucketDedup (const MgBucketArgs &a, bool packed, unsigned threads, unsigned grid, U32 perBlock, size_t lds, hipStream_t st);   /* oversize buckets planned and reduced, then both dedup instances */
MgStatus mgUniqStats (const U32 *uniqCount, U32 nBuckets, unsigned long long *out, hipStream_t st);
MgStatus mgRankLookup (const MgBucketArgs &a, hipStream_t st);
MgStatus mgBucketMerge (const MgBucketArgs &a, U64 fullest, unsigned threads, unsigned grid, U32 perBlock, size_t lds, hipStream_t st);   /* fullest: the longest list a bucket may have */

/* ---- host side ---- */
#define MG_TABLE_HIDDEN __attribute__ ((visibility ("hidden")))      /* shared by these files, not one of the library's names */
static inline unsigned mgGridWide (U64 n) { return mgGrid (n, 256, 16384); }      /* the table's kernels take up to 16384 workgroups */
static inline MgGeom mgGeomOf (const MgTable *t) { MgGeom g; g.R = t->R; g.log2NB = t->log2NB; g.kbits = t->kbits; return g; }
static inline void mgTableSetGeom (MgTable *t, int log2NB, U32 R) { t->log2NB = log2NB; t->R = R; t->nSlots = (U64) R << log2NB; }
/* the next array of a scratch layout: count elements of T at base + *at, *at moved behind them to the next 256-byte boundary.  base 0: 0, the
   layout is only measured */
template <class T> static inline T *mgCarve (void *base, size_t *at, U64 count)
{ T *p = base ? reinterpret_cast<T *> ((char *) base + *at) : 0; *at += mgAl256 (count * sizeof (T)); return p; }

/* ---- the ordered flag count (mg_rank.hip): n flags in, their number in counters[0], an index for every flagged ordinal ---- */
struct MgRankBufs { unsigned char *flags; U64 *unitCount, *unitBase; MgRankGrp *grp; };      /* [n] the flags; per rank unit: its flags, the flags before it; per 64 ordinals: the rank record */
MG_TABLE_HIDDEN size_t mgRankCarve (void *base, U64 n, MgRankBufs *r);      /* the buffers at base (256-byte aligned) for n flags; returns their bytes.  base 0: only that */
MG_TABLE_HIDDEN MgStatus mgRankCount (MgTable *t, const MgRankBufs &r, U64 n, hipStream_t st);      /* r.flags -> r.unitBase, counters[0] */
MG_TABLE_HIDDEN MgStatus mgRankRecord (const MgRankBufs &r, U64 n, hipStream_t st);                /* -> r.grp */
MG_TABLE_HIDDEN MgStatus mgRankAssignDirect (MgTable *t, const MgRankBufs &r, const U64 *dKmer, const U32 *slotId, U64 n, hipStream_t st);   /* -> value[], the slots' indices */
MG_TABLE_HIDDEN MgStatus mgRankAssignPrune (MgTable *t, const MgRankBufs &r, U64 n, U64 *dNewValue, hipStream_t st);                          /* -> dNewValue[], r.grp */
MG_TABLE_HIDDEN MgStatus mgWriteValues (MgTable *t, const MgRankGrp *grp, const U64 *dKmer, const MgSegSrc *segSrc, const MgSubSeg *subSeg, U64 n, bool aside, hipStream_t st);   /* r.grp -> value[] */
/* the element format of the partition passes (MgPartFmt) for a batch of n, and whether an element fits one packed word: mg_table.hip */
MgPartFmt mgPartFmtOf (const MgTable *t, U64 n, int hiB);
bool mgPartFmtFits (const MgTable *t, const MgPartFmt &f);
/* threads of a workgroup of the bucket kernels: by the bucket's size (knobOrZero != 0: MODGPU_BUCKET_T instead), and enough of them for
   the dedup kernel's closing sweep, MG_DEDUP_PER slots a thread */
static inline unsigned mgBucketThreads (U32 R, int knobOrZero)
{
  unsigned thr = knobOrZero ? (unsigned) knobOrZero : (R >= 4096 ? 1024u : (R >= 2048 ? 512u : 256u));
  while (thr < 1024 && (U64) thr * MG_DEDUP_PER < R) thr *= 2;
  return thr;
}
/* the grid of a kernel whose workgroups take *perBlock consecutive buckets each: 4096 workgroups at most */
static inline unsigned mgBucketGrid (U64 NB, U32 *perBlock)
{
  const unsigned grid = (unsigned) (NB < 4096 ? NB : 4096);
  *perBlock = (U32) ((NB + grid - 1) / grid);
  return (unsigned) ((NB + *perBlock - 1) / *perBlock);
}
/* f (SUB as a std::integral_constant) for the sub-chunk size `sub` a partition pass ran with: its kernels and the pulls take it as a template parameter */
template <class F> static inline void mgForSub (U32 sub, F f)
{ if (sub == MG_PART_SUB_BIG) f (std::integral_constant<int, MG_PART_SUB_BIG> ()); else f (std::integral_constant<int, MG_PART_SUB> ()); }
/* the same for a flag that is a kernel's template argument: f (std::true_type or std::false_type), and the status it returns */
template <class F> static inline MgStatus mgForFlag (bool b, F f) { return b ? f (std::true_type ()) : f (std::false_type ()); }

#endif
