/* mg_part.hip — the radix partition of the device modset table (mg_table.hip, "bucketed", step 1): a batch's (k-mer, ordinal)
 * elements sorted by bucket id in one or two streaming passes.  mgTableAdd (mg_tableadd.hip) runs both passes; the partitioned lookups (mg_find.hip) run
 * the same passes and have the scatter kernel note where every sub-chunk's runs went.  Formats and arguments: mg_table.h. */
#include "mg_table.h"

/* ======================================================================================== */
/* bucketed path, step 1: radix partition of (kmer, ordinal) by bucket id                     */

/* subSeg[] (MgSubSeg) for a batch of n in the scan's segments */
__global__ void mgSubSegKernel (const MgSegSrc src, U64 n, U32 sub, MgSubSeg *__restrict__ subSeg)
{
  const U64 q = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  if (q * sub >= n) return;
  const U32 w = mgSegOfOrdinal (src, q * sub);
  MgSubSeg e; e.w = w; e.s0 = src.segStart[w]; e.s1 = src.segStart[w + 1];
  subSeg[q] = e;
}

__global__ __launch_bounds__ (MG_PART_MAXBINS)
void mgPartChunksKernel (const U64 *__restrict__ segStart, U32 nSeg, U32 chunkElems, U32 *__restrict__ chunkBase)
{
  __shared__ U32 sS[MG_PART_MAXBINS];
  const U32 t = threadIdx.x;
  U32 c = t < nSeg ? (U32) ((segStart[t + 1] - segStart[t] + chunkElems - 1) / chunkElems) : 0;
  sS[t] = c;
  __syncthreads ();
  for (int off = 1 ; off < MG_PART_MAXBINS ; off <<= 1)
    { U32 v = t >= (U32) off ? sS[t - off] : 0;
      __syncthreads ();
      sS[t] += v;
      __syncthreads ();
    }
  if (t < nSeg) chunkBase[t] = sS[t] - c;
  if (t == nSeg - 1) chunkBase[nSeg] = sS[t];
  /* the segment of every chunk: all threads share the chunks; sS[] holds the inclusive prefix, so the segment
     of chunk q is the first s with sS[s] > q */
  const U32 total = sS[(nSeg ? nSeg : 1) - 1];
  for (U32 q = t ; q < total ; q += MG_PART_MAXBINS)
    { U32 a = 0, b = nSeg - 1;
      while (a < b) { U32 m = (a + b) / 2; if (sS[m] > q) b = m; else a = m + 1; }
      chunkBase[MG_CHUNK_SEG_AT + q] = a;
    }
}

template <int MODE>
__global__ __launch_bounds__ (256)
void mgPartHistKernel (const U64 *__restrict__ kIn, MgGeom g, MgPartFmt f, int shift, U32 nBins,
                       const U64 *__restrict__ segStart, const U32 *__restrict__ chunkBase, U32 nSeg, U32 chunkElems,
                       U32 *__restrict__ binCount)
{
  MG_BUILD_PRIO ();
  __shared__ U32 sH[MG_PART_MAXBINS];
  /* a workgroup takes a contiguous run of chunks and adds its LDS counts to the global ones only when the
     segment changes (one workgroup per chunk meant thousands of atomics on each of a few hundred addresses) */
  const U32 nChunks = chunkBase[nSeg];
  const U32 per = (nChunks + gridDim.x - 1) / gridDim.x;
  U32 c = blockIdx.x * per;
  const U32 cEnd = c + per < nChunks ? c + per : nChunks;
  if (c >= cEnd) return;
  for (U32 b = threadIdx.x ; b < nBins ; b += 256) sH[b] = 0;
  __syncthreads ();
  U32 curSeg = 0xffffffffu;
  for ( ; c < cEnd ; ++c)
    { U32 seg; U64 lo, hi;
      if (!mgChunkRange (segStart, chunkBase, nSeg, chunkElems, c, &seg, &lo, &hi)) break;
      if (seg != curSeg && curSeg != 0xffffffffu)
        { __syncthreads ();
          for (U32 b = threadIdx.x ; b < nBins ; b += 256) { U32 v = sH[b]; if (v) { atomicAdd (&binCount[(U64) curSeg * nBins + b], v); sH[b] = 0; } }
          __syncthreads ();
        }
      curSeg = seg;
      /* eight loads per lane in flight before the first LDS add */
      for (U64 i0 = lo ; i0 < hi ; i0 += 8 * 256)
        { U64 v[8];
#pragma unroll
          for (int j = 0 ; j < 8 ; ++j) { U64 i = i0 + (U64) j * 256 + threadIdx.x; v[j] = i < hi ? kIn[i] : 0; }
#pragma unroll
          for (int j = 0 ; j < 8 ; ++j)
            { U64 i = i0 + (U64) j * 256 + threadIdx.x;
              if (i < hi) atomicAdd (&sH[mgDigitOf<MODE> (v[j], g, f, shift, nBins - 1)], 1u);
            }
        }
    }
  __syncthreads ();
  if (curSeg != 0xffffffffu)
    for (U32 b = threadIdx.x ; b < nBins ; b += 256) if (sH[b]) atomicAdd (&binCount[(U64) curSeg * nBins + b], sH[b]);
}

/* the same counts from the digit bytes the pass before left beside its output (mgPartScatterKernel dOut) */
__global__ __launch_bounds__ (256)
void mgPartHistBytesKernel (const unsigned char *__restrict__ dIn, U32 nBins,
                            const U64 *__restrict__ segStart, const U32 *__restrict__ chunkBase, U32 nSeg, U32 chunkElems,
                            U32 *__restrict__ binCount)
{
  MG_BUILD_PRIO ();
  __shared__ U32 sH[MG_PART_MAXBINS];
  const U32 nChunks = chunkBase[nSeg];
  const U32 per = (nChunks + gridDim.x - 1) / gridDim.x;
  U32 c = blockIdx.x * per;
  const U32 cEnd = c + per < nChunks ? c + per : nChunks;
  if (c >= cEnd) return;
  for (U32 b = threadIdx.x ; b < nBins ; b += 256) sH[b] = 0;
  __syncthreads ();
  U32 curSeg = 0xffffffffu;
  for ( ; c < cEnd ; ++c)
    { U32 seg; U64 lo, hi;
      if (!mgChunkRange (segStart, chunkBase, nSeg, chunkElems, c, &seg, &lo, &hi)) break;
      if (seg != curSeg && curSeg != 0xffffffffu)
        { __syncthreads ();
          for (U32 b = threadIdx.x ; b < nBins ; b += 256) { U32 v = sH[b]; if (v) { atomicAdd (&binCount[(U64) curSeg * nBins + b], v); sH[b] = 0; } }
          __syncthreads ();
        }
      curSeg = seg;
      /* the unaligned head byte by byte, then four digits a load */
      U64 i0 = lo;
      const U64 head = ((lo + 3) & ~(U64) 3) < hi ? ((lo + 3) & ~(U64) 3) : hi;
      if (i0 + threadIdx.x < head) atomicAdd (&sH[dIn[i0 + threadIdx.x]], 1u);
      i0 = head;
      const U64 nWords = (hi - i0) >> 2;
      const U32 *w = reinterpret_cast<const U32 *> (dIn + i0);
      for (U64 q0 = 0 ; q0 < nWords ; q0 += 8 * 256)
        { U32 v[8];
#pragma unroll
          for (int j = 0 ; j < 8 ; ++j) { const U64 q = q0 + (U64) j * 256 + threadIdx.x; v[j] = q < nWords ? w[q] : 0; }
#pragma unroll
          for (int j = 0 ; j < 8 ; ++j)
            { const U64 q = q0 + (U64) j * 256 + threadIdx.x;
              if (q < nWords)
                { atomicAdd (&sH[v[j] & 255u], 1u); atomicAdd (&sH[(v[j] >> 8) & 255u], 1u); atomicAdd (&sH[(v[j] >> 16) & 255u], 1u); atomicAdd (&sH[v[j] >> 24], 1u); }
            }
        }
      const U64 tail = i0 + (nWords << 2);
      if (tail + threadIdx.x < hi) atomicAdd (&sH[dIn[tail + threadIdx.x]], 1u);
    }
  __syncthreads ();
  if (curSeg != 0xffffffffu)
    for (U32 b = threadIdx.x ; b < nBins ; b += 256) if (sH[b]) atomicAdd (&binCount[(U64) curSeg * nBins + b], sH[b]);
}

/* per segment: binStart = segStart + exclusive scan of its bin counts; cursor = binStart */
__global__ __launch_bounds__ (MG_PART_MAXBINS)
void mgPartScanKernel (const U32 *__restrict__ binCount, U32 nBins, const U64 *__restrict__ segStart,
                       U64 *__restrict__ binStart, unsigned long long *__restrict__ cursor, U32 cstride, U32 nSeg, U64 n)
{
  __shared__ U32 sS[MG_PART_MAXBINS];
  const U32 seg = blockIdx.x, t = threadIdx.x;
  U32 c = t < nBins ? binCount[(U64) seg * nBins + t] : 0;
  sS[t] = c;
  __syncthreads ();
  for (int off = 1 ; off < MG_PART_MAXBINS ; off <<= 1)
    { U32 v = t >= (U32) off ? sS[t - off] : 0;
      __syncthreads ();
      sS[t] += v;
      __syncthreads ();
    }
  if (t < nBins)
    { U64 st = segStart[seg] + (sS[t] - c);
      binStart[(U64) seg * nBins + t] = st;
      cursor[((U64) seg * nBins + t) * cstride] = st;
    }
  if (seg == nSeg - 1 && t == 0) binStart[(U64) nSeg * nBins] = n;
}

/* Scatter with LDS staging: a sub-chunk of 4096 elements is counting-sorted by bin in LDS, so the
 * elements of one bin leave as one contiguous run written by consecutive lanes (plain scattered
 * 8-byte stores ran at ~22 G/s: 9 ms per 1.5e8 elements for the two passes). */
/* the elements [sub, subHi) of a sub-chunk into registers, MG_PART_THREADS apart */
template <int INMODE, int SUB>
__device__ __forceinline__ void mgPartFetch (U64 *km, U32 *tk, const U64 *__restrict__ kIn, const U32 *__restrict__ tIn,
                                             const MgSegSrc &src, const MgSubSeg *__restrict__ subSeg, U64 sub, U64 subHi, int tid)
{
  if (INMODE == MG_EL_SEG)
    { const U32 wave = (U32) __builtin_amdgcn_readfirstlane (tid >> 6);
      const int lane = tid & 63;
      MgSegCursor cur;
      mgSegCursorFrom (subSeg, sub / MG_PART_SUB, &cur);            /* the first partition pass has one segment [0, n): sub is a multiple of MG_PART_SUB */
#pragma unroll
      for (int j = 0 ; j < SUB / MG_PART_THREADS ; ++j)
        { const U64 o0 = sub + (U64) j * MG_PART_THREADS + (U64) wave * 64;
          if (o0 >= subHi) break;                                     /* uniform */
          mgSegCursorSeek (src, &cur, o0);
          const U64 i = o0 + (U64) lane;
          const U64 *at = mgSegAddr (src, cur, i, o0 + 63 < subHi ? o0 + 63 : subHi - 1);
          if (i < subHi) km[j] = *at;
        }
      return;
    }
#pragma unroll
  for (int j = 0 ; j < SUB / MG_PART_THREADS ; ++j)
    { U64 i = sub + (U64) j * MG_PART_THREADS + tid;
      if (i < subHi) { km[j] = kIn[i]; if (INMODE == MG_EL_WIDE) tk[j] = tIn[i]; }
    }
}

template <int INMODE, bool PACKOUT, int SUB>     /* INMODE: what kIn holds; PACKOUT: one packed word out, otherwise (mixed k-mer, ordinal); SUB: elements of a sub-chunk */
__global__ __launch_bounds__ (MG_PART_THREADS)
void mgPartScatterKernel (const U64 *__restrict__ kIn, const U32 *__restrict__ tIn, const MgSegSrc src, const MgSubSeg *__restrict__ subSeg,
                          MgGeom g, MgPartFmt f, int shift, U32 nBins,
                          const U64 *__restrict__ segStart, const U32 *__restrict__ chunkBase, U32 nSeg, U32 chunkElems,
                          unsigned long long *__restrict__ cursor, U32 cstride, U64 *__restrict__ kOut, U32 *__restrict__ tOut,
                          unsigned long long *__restrict__ runTab, int runMode, unsigned char *__restrict__ dOut, int dShift, U32 dMask)
{
  /* dOut (the first of two passes): the NEXT pass's digit of every element, one byte each, at the element's place -- the next pass
     counts its digits from these bytes instead of reading the 8-byte elements a second time (config 2: 0.28 -> 0.06 ms) */
  /* runMode (with runTab, the partitioned lookup): 0 = the run table's rows are the sub-chunks of ONE segment (row = sub / SUB);
     1 = the second level: rows are (chunk, half) = 2 c + (sub - lo) / SUB, and every element's ordinal field is replaced by its
     position in kIn -- where its result has to go back to */
  MG_BUILD_PRIO ();
  constexpr bool WIDE = !PACKOUT;
  constexpr bool BIG = SUB > MG_PART_SUB;
  constexpr int PER = SUB / MG_PART_THREADS;
  constexpr int BINS = BIG ? MG_PART_BIG_BINS : MG_PART_MAXBINS;
  static_assert (!BIG || PACKOUT, "large sub-chunks: packed elements only");
  typedef typename std::conditional<BIG, unsigned char, unsigned short>::type Digit;
  __shared__ U64 stK[SUB];
  __shared__ U32 stT[WIDE ? SUB : 1];
  __shared__ Digit stB[SUB];
  __shared__ U32 sH[BINS], sOff[BINS];
  __shared__ unsigned long long sBase[BINS];
  __shared__ U32 sWave[MG_PART_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const U64 remMask = f.remBits >= 64 ? ~0ull : (((U64) 1 << f.remBits) - 1);
  /* A workgroup walks chunks blockIdx.x, blockIdx.x + gridDim.x, ... sub-chunk by sub-chunk, and the elements
     of the next sub-chunk are already on their way into registers while the current one is written out (one
     workgroup fills a CU's LDS, so nothing else would hide that latency). */
  U32 c = blockIdx.x, seg; U64 lo, hi;
  bool have = mgChunkRange (segStart, chunkBase, nSeg, chunkElems, c, &seg, &lo, &hi);
  U64 sub = have ? lo : 0;
  U64 km[PER]; U32 tk[PER];
#pragma unroll
  for (int j = 0 ; j < PER ; ++j) { km[j] = 0; tk[j] = 0; }
  if (have)
    { const U64 subHi = sub + SUB < hi ? sub + SUB : hi;
      mgPartFetch<INMODE, SUB> (km, tk, kIn, tIn, src, subSeg, sub, subHi, tid);
    }
  while (have)
    { const U64 subHi = sub + SUB < hi ? sub + SUB : hi;
      const U32 cnt = (U32) (subHi - sub);
      /* what comes after this sub-chunk */
      U32 nc = c, nseg = seg; U64 nlo = lo, nhi = hi, nsub = sub + SUB; bool nhave = true;
      if (nsub >= hi) { nc = c + gridDim.x; nhave = mgChunkRange (segStart, chunkBase, nSeg, chunkElems, nc, &nseg, &nlo, &nhi); nsub = nlo; }
      for (U32 b = tid ; b < nBins ; b += MG_PART_THREADS) sH[b] = 0;
      __syncthreads ();
      U32 dr[PER];
#pragma unroll
      for (int j = 0 ; j < PER ; ++j)
        { U64 i = sub + (U64) j * MG_PART_THREADS + tid;
          dr[j] = 0xffffffffu;
          if (i < subHi)
            { constexpr bool FIRST = INMODE == MG_EL_DENSE || INMODE == MG_EL_SEG;
              if (FIRST)                                         /* into mixed space, once */
                { km[j] = mgMixK (km[j], g.kbits); tk[j] = (U32) i; }
              U32 d = mgDigitOf<(FIRST ? MG_EL_WIDE : INMODE)> (km[j], g, f, shift, nBins - 1);
              dr[j] = (d << 16) | atomicAdd (&sH[d], 1u);        /* rank within (sub-chunk, bin) */
              if (FIRST && PACKOUT) km[j] = ((km[j] & remMask) << f.ordBits) | (U64) tk[j];
              if (INMODE == MG_EL_PACKED && runMode == 1) km[j] = ((km[j] >> f.ordBits) << f.ordBits) | i;
            }
        }
      __syncthreads ();
      /* exclusive scan of the bin counts (two bins per thread) + reservation of the output runs */
      unsigned long long base0 = 0, base1 = 0;
      { U32 c0 = (U32) (2 * tid) < nBins ? sH[2 * tid] : 0, c1 = (U32) (2 * tid + 1) < nBins ? sH[2 * tid + 1] : 0;
        const U32 pair = c0 + c1, incl = mgWaveInclusiveSum (pair);
        if (lane == 63) sWave[wave] = incl;
        __syncthreads ();
        U32 wb = 0;
#pragma unroll
        for (int w = 0 ; w < MG_PART_THREADS / 64 ; ++w) if (w < wave) wb += sWave[w];
        U32 ex = wb + incl - pair;
        /* the two reservations are global atomics that return a value (a microsecond or two): they are issued here
           and only waited for after the staging below, which does not need them */
        if ((U32) (2 * tid) < nBins)
          { sOff[2 * tid] = ex;
            if (c0) base0 = atomicAdd (&cursor[((U64) seg * nBins + 2 * tid) * cstride], (unsigned long long) c0);
          }
        if ((U32) (2 * tid + 1) < nBins)
          { sOff[2 * tid + 1] = ex + c0;
            if (c1) base1 = atomicAdd (&cursor[((U64) seg * nBins + 2 * tid + 1) * cstride], (unsigned long long) c1);
          }
      }
      __syncthreads ();
#pragma unroll
      for (int j = 0 ; j < PER ; ++j)
        if (dr[j] != 0xffffffffu)
          { U32 d = dr[j] >> 16, p = sOff[d] + (dr[j] & 0xffffu);
            stK[p] = km[j]; if (WIDE) stT[p] = tk[j]; stB[p] = (Digit) d;
          }
      if ((U32) (2 * tid) < nBins) sBase[2 * tid] = base0;
      if ((U32) (2 * tid + 1) < nBins) sBase[2 * tid + 1] = base1;
      if (runTab)                                          /* (uniform; the partitioned lookup) where this sub-chunk's run of every bin went, and its length */
        { const U64 row = (runMode == 1 ? 2 * (U64) c + (sub - lo) / SUB : sub / SUB) * nBins;
          if ((U32) (2 * tid) < nBins) runTab[row + 2 * tid] = base0 | ((unsigned long long) sH[2 * tid] << 40);
          if ((U32) (2 * tid + 1) < nBins) runTab[row + 2 * tid + 1] = base1 | ((unsigned long long) sH[2 * tid + 1] << 40);
        }
      /* the registers are free: fetch the next sub-chunk */
      if (nhave)
        { const U64 nsubHi = nsub + SUB < nhi ? nsub + SUB : nhi;
          mgPartFetch<INMODE, SUB> (km, tk, kIn, tIn, src, subSeg, nsub, nsubHi, tid);
        }
      __syncthreads ();
      for (U32 p = tid ; p < cnt ; p += MG_PART_THREADS)
        { U32 d = stB[p];
          U64 at = sBase[d] + (p - sOff[d]);
          kOut[at] = stK[p];                               /* plain stores: the runs of a bin are short, the L2 combines them (non-temporal: 1.5 -> 1.85 ms) */
          if (WIDE) tOut[at] = stT[p];
          if (dOut) dOut[at] = (unsigned char) mgDigitOf<(PACKOUT ? MG_EL_PACKED : MG_EL_WIDE)> (stK[p], g, f, dShift, dMask);   /* (uniform) */
        }
      __syncthreads ();
      c = nc; seg = nseg; lo = nlo; hi = nhi; sub = nsub; have = nhave;
    }
}

/* ======================================================================================== */
/* host side: one partition pass (MgPartPassArgs, mg_table.h)                                 */

MgStatus mgPartPass (const MgTable *t, MgPartPassArgs &p, hipStream_t st)
{
  MgGeom g = mgGeomOf (t);
  MgSegSrc src = {};
  if (p.inMode == MG_EL_SEG)
    { if (!p.segSrc || !p.subSeg || !p.counted) { mgSetError ("internal: segment input needs its counts"); return MG_ERR_ARG; }
      src = *p.segSrc;
      const U64 nSub = (p.n + MG_PART_SUB - 1) / MG_PART_SUB;
      MG_LAUNCH (MG_K_PART, st, mgSubSegKernel, dim3 ((unsigned) ((nSub + 255) / 256)), dim3 (256), 0, st, src, p.n, (U32) MG_PART_SUB, p.subSeg);
    }
  if (p.counted) MG_HIP (hipMemcpy2DAsync (p.binCount, sizeof (U32), p.counted, MG_HIST_STRIDE * sizeof (U32), sizeof (U32), p.nBins, hipMemcpyDeviceToDevice, st));   /* the scan counted them */
  else MG_HIP (hipMemsetAsync (p.binCount, 0, (size_t) p.nSeg * p.nBins * sizeof (U32), st));
  /* large sub-chunks where the kernel has them: packed elements, at most 256 bins */
  const int bigEnv = mgKnobs ()->partBig == MG_KNOB_UNSET ? 1 : (int) mgKnobs ()->partBig;      /* test knob: 0 = sub-chunks of MG_PART_SUB everywhere */
  const bool big = bigEnv && p.packed && p.nBins <= MG_PART_BIG_BINS && MG_PART_THREADS == 1024;
  p.subElems = (U32) (big ? MG_PART_SUB_BIG : MG_PART_SUB);
  const U32 chunkElems = 2u * p.subElems;
  MG_LAUNCH (MG_K_PART, st, mgPartChunksKernel, dim3 (1), dim3 (MG_PART_MAXBINS), 0, st, p.segStart, p.nSeg, chunkElems, p.chunkBase);
  const unsigned maxChunks = p.maxChunks = (unsigned) (p.n / chunkElems + p.nSeg + 1);
  const int sgEnv = mgKnobs ()->scatterGrid == MG_KNOB_UNSET ? 0 : (int) mgKnobs ()->scatterGrid;   /* dev knob */
  unsigned scatterGrid = maxChunks < (unsigned) (sgEnv > 0 ? sgEnv : 1024) ? maxChunks : (unsigned) (sgEnv > 0 ? sgEnv : 1024);
  const dim3 hg (maxChunks < 4096 ? maxChunks : 4096), sg (scatterGrid);
  if (!p.counted && p.digitIn)
    MG_LAUNCH (MG_K_PART_HIST, st, mgPartHistBytesKernel, hg, dim3 (256), 0, st, p.digitIn, p.nBins, p.segStart, p.chunkBase, p.nSeg, chunkElems, p.binCount);
  else if (!p.counted)
    {
#define MG_HIST(IN) MG_LAUNCH (MG_K_PART_HIST, st, mgPartHistKernel<IN>, hg, dim3 (256), 0, st, p.kIn, g, p.f, p.shift, p.nBins, p.segStart, p.chunkBase, p.nSeg, chunkElems, p.binCount)
      if (p.inMode == MG_EL_DENSE) MG_HIST (MG_EL_DENSE); else if (p.inMode == MG_EL_WIDE) MG_HIST (MG_EL_WIDE); else MG_HIST (MG_EL_PACKED);
#undef MG_HIST
    }
  /* one segment (the first pass): every workgroup reserves in the same few hundred cursors -- one cache line each
     (scatter 0.88 -> 0.73 ms: returning atomics on cursors that share a line queue behind each other) */
  const U32 cstride = p.nSeg == 1 ? 16u : 1u;                  /* (the second pass's 65536 cursors: no gain from padding) */
  MG_LAUNCH (MG_K_PART, st, mgPartScanKernel, dim3 (p.nSeg), dim3 (MG_PART_MAXBINS), 0, st, p.binCount, p.nBins, p.segStart, p.binStart, p.cursor, cstride, p.nSeg, p.n);
#define MG_SCATTER(IN, PK, SUB) MG_LAUNCH (MG_K_PART_SCATTER, st, (mgPartScatterKernel<IN, PK, SUB>), sg, dim3 (MG_PART_THREADS), 0, st, \
                                           p.kIn, p.tIn, src, p.subSeg, g, p.f, p.shift, p.nBins, p.segStart, p.chunkBase, p.nSeg, chunkElems, p.cursor, cstride, p.kOut, p.tOut, p.runTab, p.runMode, \
                                           p.digitOut, p.nextShift, p.nextBins ? p.nextBins - 1 : 0u)
#define MG_SCATTER_P(IN) mgForSub (p.subElems, [&] (auto S) { MG_SCATTER (IN, true, decltype (S)::value); })
  if (p.inMode == MG_EL_DENSE) { if (p.packed) MG_SCATTER_P (MG_EL_DENSE); else MG_SCATTER (MG_EL_DENSE, false, MG_PART_SUB); }
  else if (p.inMode == MG_EL_SEG) { if (p.packed) MG_SCATTER_P (MG_EL_SEG); else MG_SCATTER (MG_EL_SEG, false, MG_PART_SUB); }
  else if (p.inMode == MG_EL_WIDE) MG_SCATTER (MG_EL_WIDE, false, MG_PART_SUB);
  else MG_SCATTER_P (MG_EL_PACKED);
#undef MG_SCATTER_P
#undef MG_SCATTER
  MG_HIP (hipGetLastError ());
  return MG_OK;
}
