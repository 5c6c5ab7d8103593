/* mg_bucket.hip — the one-workgroup-per-bucket kernels of the device modset table's bucketed build (mg_table.hip, steps 2, 3b and 4):
 * oversize buckets reduced chunk by chunk (mgHot*), dedup, rank lookups, merge; and their launches, which mgTableAdd (mg_tableadd.hip) calls in that order, the ordered flag count
 * (step 3, mg_rank.hip) between the dedup and the lookups.
 * MgBucketArgs, mgLdsClaim and the kernels' constants: mg_table.h. */
#include "mg_table.h"

/* ======================================================================================== */
/* bucketed path, steps 2 and 4: one workgroup per bucket, the bucket lives in LDS             */

/* Both bucket kernels run a workgroup over a contiguous range of buckets.  Per bucket there is
 * little arithmetic and several dependent global round trips (bounds -> elements -> rank record),
 * so the next bucket's bounds and first elements are fetched into registers while the current
 * bucket is processed, and the LDS image is kept all-zero between buckets by clearing exactly the
 * slots the closing sweep visits (no 64 KiB re-zeroing per bucket). */

/* step 2: dedup the bucket's occurrences; uniques written in place over the bucket's range */
/* one occurrence of bucket b -> (mixed k-mer, ordinal) */
template <bool PACKED>
__device__ __forceinline__ void mgOccurrence (const MgBucketArgs &a, U32 b, U64 x, U32 t, U64 *m, U32 *ord)
{
  if (PACKED)
    { *ord = (U32) (x & (((U64) 1 << a.f.ordBits) - 1));
      *m = ((U64) (b >> a.f.loB) << a.f.remBits) | (x >> a.f.ordBits);     /* the bin's coarse digit in front of rem */
    }
  else { *m = x; *ord = t; }
}

/* one more occurrence (ordinal ord) of the k-mer in LDS slot at: the earliest ordinal wins the slot's token (assigned
 * entries carry bit 31 and stay as they are).  markDup: whoever loses -- this occurrence, or the one that held the token --
 * is not a first occurrence of a new k-mer: its flag is cleared */
__device__ __forceinline__ void mgDedupCount (const MgBucketArgs &a, U32 *sOrd, U32 *sCnt, U32 at, U32 ord)
{
  const U32 tok = mgToken (ord);
  if (a.markDup)
    { const U32 old = atomicMax (&sOrd[at], tok);
      const U32 loser = old > tok ? tok : old;
      if (loser MG_ABLATE_AND (!(a.debug & 1))) a.flags[0x7fffffffu - loser] = 0;
    }
  else atomicMax (&sOrd[at], tok);
  atomicAdd (&sCnt[at], 1u);
}
/* inclusive prefix max over the 64 lanes of a wave (DPP, the steps of mgWaveInclusiveSum; lanes without a source take 0; every lane
   must be active), and the largest value of them all */
__device__ __forceinline__ U32 mgWavePrefixMax (U32 v)
{
#define MG_MAX_DPP(ctrl, rows) do { const U32 o_ = (U32) __builtin_amdgcn_update_dpp (0, (int) v, ctrl, rows, 0xf, false); v = o_ > v ? o_ : v; } while (0)
  MG_MAX_DPP (0x111, 0xf); MG_MAX_DPP (0x112, 0xf); MG_MAX_DPP (0x114, 0xf); MG_MAX_DPP (0x118, 0xf); MG_MAX_DPP (0x142, 0xa); MG_MAX_DPP (0x143, 0xc);
#undef MG_MAX_DPP
  return v;
}
__device__ __forceinline__ U32 mgWaveMax (U32 v) { return (U32) __builtin_amdgcn_readlane ((int) mgWavePrefixMax (v), 63); }
/* A bucket's occurrences beyond the ones fetched ahead -- only a bucket with a k-mer of very many copies has any (a poly-A
 * 21-mer is a modimizer at k = 21, d = 64, seed 17, and a human read set holds millions of them): a wave takes 64 of them at a
 * time, and the lanes that landed in the same slot as its first lane are counted as ONE occurrence with their number -- the
 * earliest of them stands for all at the slot's token, the others are not first occurrences (markDup: their flags are
 * cleared) -- instead of 64 atomics queueing on one LDS word (1.7 ns per occurrence: 1.7 s for a batch of nothing but poly-A).
 * Every lane of the wave calls this, `live` or not. */
__device__ __forceinline__ void mgDedupCountWave (const MgBucketArgs &a, U32 *sOrd, U32 *sCnt, U32 R, bool live, U32 at, U32 ord)
{
  live = live && at < R;
  const U32 at0 = (U32) __builtin_amdgcn_readfirstlane ((int) at);
  const bool mine = live && at == at0;
  const U32 n = (U32) __popcll (__ballot (mine));
  if (n > 1)                                                   /* (uniform) */
    { const U32 tok = mgToken (ord);
      const U32 best = mgWaveMax (mine ? tok : 0u);
      if (mine)
        { if (tok == best)
            { const U32 old = atomicMax (&sOrd[at], tok);
              if (a.markDup) { const U32 loser = old > tok ? tok : old; if (loser) a.flags[0x7fffffffu - loser] = 0; }
              atomicAdd (&sCnt[at], n);
            }
          else if (a.markDup) a.flags[ord] = 0;
        }
      else if (live) mgDedupCount (a, sOrd, sCnt, at, ord);
    }
  else if (live) mgDedupCount (a, sOrd, sCnt, at, ord);
}

/* A run [from, hi) of occurrences of bucket b into the LDS image, MG_HOT_DEPTH x T at a time; every lane stays in the
 * loop: the wave works together (see mgDedupCountWave).  Used by the dedup kernel for what it did not fetch ahead and by
 * mgHotReduceKernel for a chunk of an oversize bucket. */
template <bool PACKED>
__device__ __forceinline__ void mgDedupRun (const MgBucketArgs &a, U32 b, unsigned long long *sKey, U32 *sOrd, U32 *sCnt,
                                            U32 R, U32 T, U32 tid, U64 from, U64 hi)
{
  /* the occurrences beyond the ones fetched ahead (a bucket with a k-mer of very many copies), MG_HOT_DEPTH x T at a time; every
     lane stays in the loop: the wave works together */
  for (U64 i0 = from ; i0 < hi ; i0 += (U64) MG_HOT_DEPTH * T)
    { U64 x[MG_HOT_DEPTH]; U32 tx[MG_HOT_DEPTH]; bool live[MG_HOT_DEPTH];
#pragma unroll
      for (int j = 0 ; j < MG_HOT_DEPTH ; ++j)
        { const U64 i = i0 + (U64) j * T + tid;
          live[j] = i < hi;
          x[j] = live[j] ? a.pK[i] : 0; tx[j] = (!PACKED && live[j]) ? a.pT[i] : 0;
        }
      /* all of the wave's elements one k-mer (that of its first lane)?  Then one claim, one token, one count for all of them */
      const int kShift = PACKED ? a.f.ordBits : 0;
      const U64 x0 = mgUniform64 (x[0]); const U32 tx0 = (U32) __builtin_amdgcn_readfirstlane ((int) tx[0]);
      bool same = true;
#pragma unroll
      for (int j = 0 ; j < MG_HOT_DEPTH ; ++j) if (live[j] && (x[j] >> kShift) != (x0 >> kShift)) same = false;
      const bool first = __builtin_amdgcn_readfirstlane ((int) live[0]) != 0;
      bool done = false;
      if (first && __ballot (!same) == 0 MG_ABLATE_AND (!(a.debug & 6)))                     /* (uniform) */
        { U64 m; U32 o0; mgOccurrence<PACKED> (a, b, x0, tx0, &m, &o0);
          const U32 at = mgLdsClaim (sKey, R, mgHomeOfM (m, a.g), m + 1);          /* (every lane claims the same slot with the same key) */
          if (at < R)
            { U32 tok[MG_HOT_DEPTH], tmax = 0, cnt = 0;
#pragma unroll
              for (int j = 0 ; j < MG_HOT_DEPTH ; ++j)
                { const U32 ord = PACKED ? (U32) (x[j] & (((U64) 1 << a.f.ordBits) - 1)) : tx[j];
                  tok[j] = live[j] ? mgToken (ord) : 0u;
                  if (tok[j] > tmax) tmax = tok[j];
                  cnt += live[j] ? 1u : 0u;
                }
              const U32 best = mgWaveMax (tmax);
              const U32 total = (U32) __builtin_amdgcn_readlane ((int) mgWaveInclusiveSum (cnt), 63);
              if (cnt && tmax == best)                                                        /* (one lane: tokens are all different) */
                { const U32 old = atomicMax (&sOrd[at], best);
                  if (a.markDup) { const U32 loser = old > best ? best : old; if (loser) a.flags[0x7fffffffu - loser] = 0; }
                  atomicAdd (&sCnt[at], total);
                }
              if (a.markDup)
                {
#pragma unroll
                  for (int j = 0 ; j < MG_HOT_DEPTH ; ++j) if (live[j] && tok[j] != best) a.flags[0x7fffffffu - tok[j]] = 0;
                }
              done = true;
            }
        }
      if (!done)                                                                              /* (uniform) */
        {
#pragma unroll
          for (int j = 0 ; j < MG_HOT_DEPTH ; ++j)
            { U64 m = 0; U32 ord = 0, at = R;
              if (live[j])
                { mgOccurrence<PACKED> (a, b, x[j], tx[j], &m, &ord);
#ifdef MG_ABLATE
                  if (a.debug & 4) { at = mgHomeOfM (m, a.g); sKey[at] = m + 1; } else
#endif
                  at = mgLdsClaim (sKey, R, mgHomeOfM (m, a.g), m + 1);
                  if (at == R) a.counters[1] = 1;
                }
#ifdef MG_ABLATE
              if (a.debug & 2) { if (live[j] && at < R) { sOrd[at] = mgToken (ord); sCnt[at] = 1; } continue; }
#endif
              mgDedupCountWave (a, sOrd, sCnt, R, live[j], at, ord);
            }
        }
    }
}


/* the chunks of every oversize bucket, listed for mgHotReduceKernel */
__global__ __launch_bounds__ (256)
void mgHotPlanKernel (const MgBucketArgs a)
{
  const U32 b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nBuckets) return;
  const U64 cnt = a.bucketStart[b + 1] - a.bucketStart[b];
  if (cnt <= a.hotSplit) return;
  const U64 L = mgHotChunkLen (cnt, a.hotChunk);
  const U32 nCh = (U32) ((cnt + L - 1) / L);
  const U64 at = atomicAdd (a.hotCount, (unsigned long long) nCh);
  for (U32 j = 0 ; j < nCh ; ++j) a.hotItems[at + j] = ((U64) b << 32) | j;
  a.hotBuckets[atomicAdd (a.hotCount + 1, 1ull)] = b;
}

/* one chunk of an oversize bucket -> its distinct k-mers as weighted entries, in place at the chunk's start.  The LDS image
 * is the dedup kernel's (keys of ONE bucket: at most R distinct, or the bucket overflows there too); it starts empty, so a
 * k-mer's token here is its earliest ordinal within the chunk, and with markDup every other occurrence of the chunk has its
 * flag cleared right here -- none of them can be a first occurrence. */
template <bool PACKED>
__global__ __launch_bounds__ (1024)
void mgHotReduceKernel (const MgBucketArgs a)
{
  const U32 R = a.g.R, T = blockDim.x, tid = threadIdx.x;
  unsigned long long *sKey = reinterpret_cast<unsigned long long *> (mgDynLds);
  U32 *sOrd = reinterpret_cast<U32 *> (mgDynLds + (size_t) R * 8);
  U32 *sCnt = sOrd + R;
  U32 *sN = sCnt + R;
  const U64 nItems = *a.hotCount;
  if (blockIdx.x >= nItems) return;
  for (U32 i = tid ; i < R ; i += T) { sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0; }
  if (tid == 0) sN[0] = 0;
  __syncthreads ();
  for (U64 w = blockIdx.x ; w < nItems ; w += gridDim.x)
    { const U64 item = a.hotItems[w];
      const U32 b = (U32) (item >> 32), j = (U32) item;
      const U64 lo = a.bucketStart[b], hi = a.bucketStart[b + 1];
      const U64 L = mgHotChunkLen (hi - lo, a.hotChunk);
      const U64 cs = lo + (U64) j * L, ce = cs + L < hi ? cs + L : hi;
      mgDedupRun<PACKED> (a, b, sKey, sOrd, sCnt, R, T, tid, cs, ce);
      __syncthreads ();
      for (U32 i = tid ; i < R ; i += T)
        { const unsigned long long key = sKey[i];
          if (key)
            { const U32 tok = sOrd[i], c = sCnt[i];
              sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0;
              const U32 at = atomicAdd (&sN[0], 1u);
              const U32 ord = 0x7fffffffu - tok;
              if (PACKED) a.pK[cs + at] = (((key - 1) & (((U64) 1 << a.f.remBits) - 1)) << a.f.ordBits) | ord;
              else { a.pK[cs + at] = key - 1; a.pT[cs + at] = ord; }
              a.pC[cs + at] = c;
            }
        }
      __syncthreads ();
      if (tid == 0) { const U32 nc = sN[0]; if (cs + nc < ce) a.pC[cs + nc] = 0; sN[0] = 0; }
      __syncthreads ();
    }
}

/* the dedup kernel's side of it: the weighted entries of an oversize bucket's chunks into the bucket's image; a wave takes
 * chunks w, w + T / 64, ... and reads a chunk's list 64 entries at a time up to its end (pC = 0, or the chunk's end) */
template <bool PACKED>
__device__ __forceinline__ void mgDedupHotBucket (const MgBucketArgs &a, U32 b, unsigned long long *sKey, U32 *sOrd, U32 *sCnt,
                                                  U32 R, U32 T, U32 tid, U64 lo, U64 hi)
{
  const U64 L = mgHotChunkLen (hi - lo, a.hotChunk);
  const U32 nCh = (U32) ((hi - lo + L - 1) / L);
  const U32 lane = tid & 63;
  for (U32 j = tid >> 6 ; j < nCh ; j += T >> 6)
    { const U64 cs = lo + (U64) j * L, ce = cs + L < hi ? cs + L : hi;
      for (U64 base = cs ; base < ce ; base += 64)
        { const U64 i = base + lane;
          const U32 c = i < ce ? a.pC[i] : 0u;
          const unsigned long long ended = __ballot (c == 0);
          const bool live = c != 0 && (ended == 0 || lane < (U32) __builtin_ctzll (ended));
          if (live)
            { U64 m; U32 ord;
              mgOccurrence<PACKED> (a, b, a.pK[i], PACKED ? 0u : a.pT[i], &m, &ord);
              const U32 at = mgLdsClaim (sKey, R, mgHomeOfM (m, a.g), m + 1);
              if (at == R) a.counters[1] = 1;
              else
                { const U32 tok = mgToken (ord);
                  const U32 old = atomicMax (&sOrd[at], tok);
                  if (a.markDup) { const U32 loser = old > tok ? tok : old; if (loser) a.flags[0x7fffffffu - loser] = 0; }
                  atomicAdd (&sCnt[at], c);
                }
            }
          if (ended) break;
        }
    }
}

/* HOT = false: every bucket but the oversize ones; HOT = true (its own launch, a few workgroups): the oversize buckets the plan
   listed, from their chunks' weighted entries -- a second instance so that the ordinary one keeps its registers (with the walk
   inlined as a branch the dedup of config 2 went from 1.22 to 1.27 ms, as a called function to 3.2) */
template <bool PACKED, bool SLOT, int PER, bool HOT>       /* SLOT: a.slotShift != 0; PER: slots of the image per thread, R <= PER x threads */
__global__ __launch_bounds__ (1024) __attribute__ ((amdgpu_waves_per_eu (PER == MG_DEDUP_PER ? 8 : 4)))      /* 64 registers: two workgroups per CU */
void mgBucketDedupKernel (const MgBucketArgs a, U32 bucketsPerBlock)
{
  MG_BUILD_PRIO ();
  const U32 R = a.g.R, T = blockDim.x, tid = threadIdx.x;
  unsigned long long *sKey = reinterpret_cast<unsigned long long *> (mgDynLds);
  U32 *sOrd = reinterpret_cast<U32 *> (mgDynLds + (size_t) R * 8);
  U32 *sCnt = sOrd + R;
  U32 *sGrp = sCnt + R;                            /* [MG_RANK_GROUPS] members of each group of the bucket's list */
  const U32 nGrp = a.nSlices + 1;
  U32 b = blockIdx.x * bucketsPerBlock, bEnd = b + bucketsPerBlock;
  U64 hotAt = blockIdx.x; const U64 nHot = HOT ? a.hotCount[1] : 0;
  if (HOT) { if (hotAt >= nHot) return; }
  else
    { if (bEnd > a.nBuckets) bEnd = a.nBuckets;
      if (b >= bEnd) return;
    }
  for (U32 i = tid ; i < R ; i += T) { sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0; }
  if (tid < MG_RANK_GROUPS) sGrp[tid] = 0;
  for ( ; ; )                                           /* (HOT: one listed bucket per turn; otherwise a single turn over the workgroup's range) */
  {
  if (HOT) { b = a.hotBuckets[hotAt]; bEnd = b + 1; }
  U64 lo = a.bucketStart[b], hi = a.bucketStart[b + 1];
  U32 occNow = a.occ[b];                          /* fetched one bucket ahead like the bounds: it gates a branch */
  U64 ck[MG_BUCKET_PREFETCH]; U32 ct[MG_BUCKET_PREFETCH];
#pragma unroll
  for (int j = 0 ; j < MG_BUCKET_PREFETCH ; ++j)
    { U64 i = lo + (U64) j * T + tid; ck[j] = 0; ct[j] = 0; if (!HOT && i < hi) { ck[j] = __builtin_nontemporal_load (&a.pK[i]); if (!PACKED) ct[j] = __builtin_nontemporal_load (&a.pT[i]); } }
  __syncthreads ();
  for ( ; b < bEnd ; ++b)
    { /* fetch the next bucket while this one is processed */
      U64 nlo = hi, nhi = hi;
      U64 nk[MG_BUCKET_PREFETCH]; U32 nt[MG_BUCKET_PREFETCH];
#pragma unroll
      for (int j = 0 ; j < MG_BUCKET_PREFETCH ; ++j) { nk[j] = 0; nt[j] = 0; }
      U32 occNext = 0;
      if (b + 1 < bEnd)
        { nhi = a.bucketStart[b + 2];
          occNext = a.occ[b + 1];
#pragma unroll
          for (int j = 0 ; j < MG_BUCKET_PREFETCH ; ++j)
            { U64 i = nlo + (U64) j * T + tid; if (i < nhi) { nk[j] = __builtin_nontemporal_load (&a.pK[i]); if (!PACKED) nt[j] = __builtin_nontemporal_load (&a.pT[i]); } }
        }
      if (hi == lo)
        { if (tid == 0) a.uniqCount[b] = 0;
          if (tid < nGrp + 1) a.sliceOff[(U64) b * (nGrp + 1) + tid] = 0;
        }
      else if (!HOT && hi - lo > a.hotSplit) { }          /* (uniform) an oversize bucket: the other instance's */
      else
        { if (occNow)
            { for (U32 i = tid ; i < R ; i += T)
                { uint4 v = *reinterpret_cast<const uint4 *> (&a.slots[(U64) b * R + i]);
                  sKey[i] = mgKeyOf (v); sOrd[i] = v.z;
                }
              __syncthreads ();
            }
          if (HOT) mgDedupHotBucket<PACKED> (a, b, sKey, sOrd, sCnt, R, T, tid, lo, hi);   /* reduced to weighted entries by mgHotReduceKernel */
          else
          {
#pragma unroll
          for (int j = 0 ; j < MG_BUCKET_PREFETCH ; ++j)
            if (lo + (U64) j * T + tid < hi)
              { U64 m; U32 ord; mgOccurrence<PACKED> (a, b, ck[j], ct[j], &m, &ord);
                U32 at;
#ifdef MG_ABLATE
                if (a.debug & 4) { at = mgHomeOfM (m, a.g); sKey[at] = m + 1; } else
#endif
                at = mgLdsClaim (sKey, R, mgHomeOfM (m, a.g), m + 1);
                if (at == R) a.counters[1] = 1;
#ifdef MG_ABLATE
                else if (a.debug & 2) { sOrd[at] = mgToken (ord); sCnt[at] = 1; }
#endif
                else { mgDedupCount (a, sOrd, sCnt, at, ord); }
              }
          /* the occurrences beyond the ones fetched ahead (a bucket with a k-mer of very many copies) */
          mgDedupRun<PACKED> (a, b, sKey, sOrd, sCnt, R, T, tid, lo + (U64) MG_BUCKET_PREFETCH * T, hi);
          }
          __syncthreads ();
          /* the uniques leave grouped (see MgBucketArgs).  Every thread takes its slots of the image into registers
             (clearing them for the next bucket) and counts the groups' members -- a unique's place inside its group is
             what the add returns; the counts become places in the list; the entries go back into the (now free) LDS
             arrays in list order, and leave from there with coalesced stores */
          unsigned long long rk[PER]; U32 rc[PER], ro[PER], rp[PER];
#pragma unroll
          for (int j = 0 ; j < PER ; ++j)
            { const U32 i = (U32) j * T + tid;
              rk[j] = 0; rc[j] = 0; ro[j] = 0; rp[j] = 0;
              if (i < R) rk[j] = sKey[i];
              if (rk[j])
                { rc[j] = sCnt[i]; ro[j] = sOrd[i];
                  sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0;
                  rk[j] = (rk[j] - 1) | (SLOT ? (unsigned long long) i << MG_SLOT_SHIFT : 0ull);   /* the list holds the mixed k-mer (key - 1), under its slot where there is room */
                  if (rc[j]) rp[j] = atomicAdd (&sGrp[mgIsAssigned (ro[j]) ? a.nSlices : ((0x7fffffffu - ro[j]) >> a.sliceShift)], 1u);
                }
            }
          __syncthreads ();
          const int lane = (int) (tid & 63);
          const U32 gv = (U32) lane < nGrp ? sGrp[lane] : 0;            /* every wave scans the counts for itself */
          const U32 gIncl = mgWaveInclusiveSum (gv);
          const U32 gBase = gIncl - gv;
          const U32 total = (U32) __builtin_amdgcn_readlane ((int) gIncl, 63);
          if (tid < 64)
            { if ((U32) lane <= nGrp) a.sliceOff[(U64) b * (nGrp + 1) + lane] = (unsigned short) gBase;     /* [nGrp]: the list's length */
              if (lane == 0) a.uniqCount[b] = total;
            }
#pragma unroll
          for (int j = 0 ; j < PER ; ++j)
            { const U32 grp = mgIsAssigned (ro[j]) ? a.nSlices : ((0x7fffffffu - ro[j]) >> a.sliceShift);
              const U32 at = (U32) __shfl ((int) gBase, (int) (rc[j] ? grp : 0)) + rp[j];
              if (rc[j]) { sKey[at] = rk[j]; sOrd[at] = ro[j]; sCnt[at] = rc[j]; }
            }
          __syncthreads ();
          if (tid < MG_RANK_GROUPS) sGrp[tid] = 0;
          for (U32 i = tid ; i < total ; i += T)
            { const U64 k = sKey[i]; const U32 ord = sOrd[i], c = sCnt[i];
              sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0;
              if (true MG_ABLATE_AND (!(a.debug & 8)))
                { __builtin_nontemporal_store (k, &a.pK[lo + i]); __builtin_nontemporal_store (ord, &a.pT[lo + i]); __builtin_nontemporal_store (c, &a.pC[lo + i]); }
              if (!a.markDup && !mgIsAssigned (ord) MG_ABLATE_AND (!(a.debug & 1))) a.flags[0x7fffffffu - ord] = 1;
            }
          __syncthreads ();
        }
      lo = nlo; hi = nhi; occNow = occNext;
#pragma unroll
      for (int j = 0 ; j < MG_BUCKET_PREFETCH ; ++j) { ck[j] = nk[j]; ct[j] = nt[j]; }
    }
  if (!HOT) break;
  hotAt += gridDim.x;
  if (hotAt >= nHot) break;
  }
}

/* ---- placement by prefix scan (the merge kernel, a bucket that was empty before the add) ----
 * All of the bucket's keys are known at once and distinct, so the linear-probing layout follows without a probe:
 *     cnt[h]   = keys whose home slot is h (a key's rank r among them: what its LDS add returns)
 *     C[h]     = exclusive prefix sum of cnt
 *     start[h] = max (h, start[h-1] + cnt[h-1]) = C[h] + max (carry, max over j <= h of (j - C[j]))
 *     slot     = (start[home] + r) mod R
 * carry is what runs over the bucket's end and comes in again at slot 0: max (0, max over all j of (j - C[j]) + N - R) for N < R
 * keys -- it never exceeds that maximum, so one pass with carry = 0 gives it and it enters as a plain max.  Keys end up ordered by
 * home slot with no empty slot between a key's home and its place: an ordinary linear-probing bucket to every reader.
 * A block of consecutive slots is summed up as (S, M) = (its keys, max of j - C[j] with C counted from the block's start); two
 * neighbours combine to (SA + SB, max (MA, MB - SA)). */
/* start[] of the bucket whose home counts stand in cnt[0..R) (every thread of the workgroup calls this after the barrier behind the
 * counting): left in sStart as 16-bit words (start < 2R <= 16384), cnt[] zeroed again; returns the carry.  n: the keys counted
 * (< R).  A thread owns `per` consecutive slots (a multiple of four: 16-byte LDS accesses), sWave: 2 x 16 words.  Ends WITHOUT a
 * barrier: the caller puts one before sStart is read. */
__device__ __forceinline__ U32 mgPlaceStarts (U32 *cnt, unsigned short *sStart, int *sWave, U32 R, U32 T, U32 tid, U32 n)
{
  const U32 per = (R + 4 * T - 1) / (4 * T) * 4;
  const U32 j0 = tid * per, j1 = j0 + per < R ? j0 + per : R;      /* (R is a multiple of MG_R_QUANTUM, so of four) */
  /* M never falls below 0 where it counts (slot 0 gives 0 - 0), so every max below is taken with 0 and the scans are the wave's
     plain sum and max: first the sums, then the maxima moved to the common origin, inside the wave and then over the waves */
  U32 vS = 0; int vM = 0;
  for (U32 j = j0 ; j < j1 ; j += 4)
    { const uint4 c = *reinterpret_cast<const uint4 *> (&cnt[j]);
      int m = (int) j - (int) vS;               vM = m > vM ? m : vM; vS += c.x;
      m = (int) (j + 1) - (int) vS;             vM = m > vM ? m : vM; vS += c.y;
      m = (int) (j + 2) - (int) vS;             vM = m > vM ? m : vM; vS += c.z;
      m = (int) (j + 3) - (int) vS;             vM = m > vM ? m : vM; vS += c.w;
    }
  const int lane = (int) (tid & 63);
  const U32 wave = (U32) __builtin_amdgcn_readfirstlane ((int) (tid >> 6));
  const U32 inS = mgWaveInclusiveSum (vS), exS = inS - vS;               /* keys before this thread inside its wave */
  const U32 inM = mgWavePrefixMax (vM > (int) exS ? (U32) vM - exS : 0u);  /* counted from the wave's first slot */
  if (lane == 63) { sWave[2 * wave] = (int) inS; sWave[2 * wave + 1] = (int) inM; }
  U32 exM = (U32) __shfl_up ((int) inM, 1);
  if (lane == 0) exM = 0;
  __syncthreads ();
  /* the waves' sums: every wave scans the (at most 16) pairs for itself, one per lane */
  U32 wS = 0, wM = 0;
  if ((U32) lane < (T + 63) / 64) { wS = (U32) sWave[2 * lane]; wM = (U32) sWave[2 * lane + 1]; }
  const U32 wInS = mgWaveInclusiveSum (wS), wExS = wInS - wS;
  const U32 wInM = mgWavePrefixMax (wM > wExS ? wM - wExS : 0u);
  const int mAll = __builtin_amdgcn_readlane ((int) wInM, 63);
  U32 beforeS = 0, beforeM = 0;
  if (wave) { beforeS = (U32) __builtin_amdgcn_readlane ((int) wInS, (int) wave - 1); beforeM = (U32) __builtin_amdgcn_readlane ((int) wInM, (int) wave - 1); }
  { const U32 m = exM > beforeS ? exM - beforeS : 0u; beforeM = beforeM > m ? beforeM : m; beforeS += exS; }
  const int over = mAll + (int) n - (int) R;
  const U32 carry = over > 0 ? (U32) over : 0u;
  U32 c = beforeS; int e = beforeM > carry ? (int) beforeM : (int) carry;
  for (U32 j = j0 ; j < j1 ; j += 4)
    { const uint4 k = *reinterpret_cast<const uint4 *> (&cnt[j]);
      *reinterpret_cast<uint4 *> (&cnt[j]) = make_uint4 (0, 0, 0, 0);
      U32 s0, s1, s2, s3; int m;
      m = (int) j - (int) c;       e = m > e ? m : e; s0 = c + (U32) e; c += k.x;
      m = (int) (j + 1) - (int) c; e = m > e ? m : e; s1 = c + (U32) e; c += k.y;
      m = (int) (j + 2) - (int) c; e = m > e ? m : e; s2 = c + (U32) e; c += k.z;
      m = (int) (j + 3) - (int) c; e = m > e ? m : e; s3 = c + (U32) e; c += k.w;
      *reinterpret_cast<uint2 *> (&sStart[j]) = make_uint2 (s0 | (s1 << 16), s2 | (s3 << 16));
    }
  return carry;
}

/* step 4: merge the bucket's uniques into the table bucket and stream it back */
template <int KEEP>          /* uniques per thread the scan placement takes (2: the ones fetched ahead, no more registers; MG_PLACE_KEEP: every list of a bucket of up to 4 x T slots) */
__global__ __launch_bounds__ (1024) __attribute__ ((amdgpu_waves_per_eu (8)))      /* 64 registers: two workgroups per CU */
void mgBucketMergeKernel (const MgBucketArgs a, U32 bucketsPerBlock)
{
  MG_BUILD_PRIO ();
  const U32 R = a.g.R, T = blockDim.x, tid = threadIdx.x;
  unsigned long long *sKey = reinterpret_cast<unsigned long long *> (mgDynLds);
  U32 *sOrd = reinterpret_cast<U32 *> (mgDynLds + (size_t) R * 8);
  U32 *sCnt = sOrd + R;
  U32 b = blockIdx.x * bucketsPerBlock, bEnd = b + bucketsPerBlock;
  if (bEnd > a.nBuckets) bEnd = a.nBuckets;
  if (b >= bEnd) return;
  for (U32 i = tid ; i < R ; i += T) { sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0; }
  U32 *sLive = sCnt + R + 4;                       /* MG_LIVE_BINS small-depth bins */
  for (U32 i = tid ; i < MG_LIVE_BINS ; i += T) sLive[i] = 0;
  int *sWave = reinterpret_cast<int *> (sLive + MG_LIVE_BINS);                            /* mgPlaceStarts: 2 x 16 words */
  unsigned short *sStart = reinterpret_cast<unsigned short *> (sWave + 32);              /* [R] */
  U32 *sPlaced = sCnt + R;                         /* [2] (thread 0's) buckets laid out by scan, and those of them that ran over their end */
  if (tid < 2) sPlaced[tid] = 0;
  U32 n1 = 0, n2 = 0;                              /* depth 1 and 2, the commonest, counted per wave */
  U32 nu = a.uniqCount[b];
  U32 nNew = a.sliceOff[(U64) b * (a.nSlices + 2) + a.nSlices];   /* the list's first nNew uniques are new to the table, the others are in it */
  U32 occNow = a.occ[b];                          /* one bucket ahead, like the counts */
  U64 lo = a.bucketStart[b];
  U64 ck[MG_MERGE_PREFETCH]; U32 co[MG_MERGE_PREFETCH], cc[MG_MERGE_PREFETCH];
#pragma unroll
  for (int j = 0 ; j < MG_MERGE_PREFETCH ; ++j)
    { const U32 i = (U32) j * T + tid; ck[j] = 0; co[j] = 0; cc[j] = 0;
      if (i < nu) { ck[j] = __builtin_nontemporal_load (&a.pK[lo + i]); co[j] = __builtin_nontemporal_load (&a.pT[lo + i]); cc[j] = __builtin_nontemporal_load (&a.pC[lo + i]); }
    }
  __syncthreads ();
  for ( ; b < bEnd ; ++b)
    { U32 nnu = 0; U64 nlo = 0; U64 nk[MG_MERGE_PREFETCH]; U32 no[MG_MERGE_PREFETCH], ncc[MG_MERGE_PREFETCH], occNext = 0, nNewNext = 0;
#pragma unroll
      for (int j = 0 ; j < MG_MERGE_PREFETCH ; ++j) { nk[j] = 0; no[j] = 0; ncc[j] = 0; }
      if (b + 1 < bEnd)
        { nnu = a.uniqCount[b + 1]; nlo = a.bucketStart[b + 1]; occNext = a.occ[b + 1];
          nNewNext = a.sliceOff[(U64) (b + 1) * (a.nSlices + 2) + a.nSlices];
#pragma unroll
          for (int j = 0 ; j < MG_MERGE_PREFETCH ; ++j)
            { const U32 i = (U32) j * T + tid;
              if (i < nnu) { nk[j] = __builtin_nontemporal_load (&a.pK[nlo + i]); no[j] = __builtin_nontemporal_load (&a.pT[nlo + i]); ncc[j] = __builtin_nontemporal_load (&a.pC[nlo + i]); }
            }
        }
      if (nu)
        {
          if (occNow)
            { for (U32 i = tid ; i < R ; i += T)
                { uint4 v = *reinterpret_cast<const uint4 *> (&a.slots[(U64) b * R + i]);
                  sKey[i] = mgKeyOf (v); sOrd[i] = v.z; sCnt[i] = v.w;
                }
              __syncthreads ();
            }
          if (!occNow && a.place && !a.slotShift)   /* (uniform) the bucket was empty: every unique is new, and all of them are here.  (With carried slots a
                                                       list entry holds its slot above the k-mer and goes where it says, below, empty bucket or not.) */
            { /* KEEP x T uniques are laid out by scan, their home and rank kept in a register each between the counting and
                 the stores (those beyond the ones fetched ahead are read again for the stores); a longer list's others -- the launcher picks KEEP so that only a
                 bucket of more than 4 x T slots, the 8192-slot table, has any -- are then claimed into the image the scan left (a valid
                 linear-probing bucket) as in the parent. */
              const U32 nScan = nu < (U32) KEEP * T ? nu : (U32) KEEP * T;
              if (nu >= R) { a.counters[1] = 1; }             /* (uniform) no room: as mgLdsClaim returning R; the bucket stays empty */
              else
                { U32 hr[KEEP];                             /* home << 16 | rank (both < R <= 8192) */
#pragma unroll
                  for (int j = 0 ; j < KEEP ; ++j)
                    { const U32 i = (U32) j * T + tid;
                      hr[j] = 0;
                      if (i < nScan MG_ABLATE_AND (!(a.debug & 512)))
                        { const U64 km = j < MG_MERGE_PREFETCH ? ck[j < MG_MERGE_PREFETCH ? j : 0] : __builtin_nontemporal_load (&a.pK[lo + i]);
                          const U32 home = mgHomeOfM (km, a.g); hr[j] = (home << 16) | atomicAdd (&sOrd[home], 1u);
                        }
                    }
                  __syncthreads ();
                  U32 carry = 0;
#ifdef MG_ABLATE
                  if (a.debug & 1024) { for (U32 i = tid ; i < R ; i += T) { sStart[i] = (unsigned short) i; sOrd[i] = 0; } } else
#endif
                  carry = mgPlaceStarts (sOrd, sStart, sWave, R, T, tid, nScan);
                  if (tid == 0) { ++sPlaced[0]; if (carry) ++sPlaced[1]; }
                  __syncthreads ();
#pragma unroll
                  for (int j = 0 ; j < KEEP ; ++j)
                    { const U32 i = (U32) j * T + tid;
                      if (i < nScan MG_ABLATE_AND (!(a.debug & 2048)))
                        { U64 km; U32 ord, c;
                          if (j < MG_MERGE_PREFETCH) { km = ck[j < MG_MERGE_PREFETCH ? j : 0]; ord = co[j < MG_MERGE_PREFETCH ? j : 0]; c = cc[j < MG_MERGE_PREFETCH ? j : 0]; }
                          else { km = __builtin_nontemporal_load (&a.pK[lo + i]); ord = __builtin_nontemporal_load (&a.pT[lo + i]); c = __builtin_nontemporal_load (&a.pC[lo + i]); }
                          U32 at = (U32) sStart[hr[j] >> 16] + (hr[j] & 0xffffu);
                          if (at >= R) at -= R;
                          sKey[at] = km + 1; sOrd[at] = ord; sCnt[at] = a.withDepth ? c : 0;
                        }
                    }
                  if (nu > nScan)                                /* (uniform) */
                    { __syncthreads ();
                      for (U32 i = nScan + tid ; i < nu ; i += T)
                        { const U64 km = __builtin_nontemporal_load (&a.pK[lo + i]);
                          const U32 at = mgLdsClaim (sKey, R, mgHomeOfM (km, a.g), km + 1);
                          if (at == R) { a.counters[1] = 1; continue; }
                          sOrd[at] = __builtin_nontemporal_load (&a.pT[lo + i]); sCnt[at] = a.withDepth ? __builtin_nontemporal_load (&a.pC[lo + i]) : 0;
                        }
                    }
                }
            }
          else
          /* the rank lookup kernel has turned the new uniques' ordinals into indices: place and count */
          for (U32 i = tid, jj = 0 ; i < nu ; i += T, ++jj)
            { U64 km; U32 ord, c;
              if (jj < MG_MERGE_PREFETCH)
                { km = ck[0]; ord = co[0]; c = cc[0];
#pragma unroll
                  for (int j = 1 ; j < MG_MERGE_PREFETCH ; ++j) if (jj == (U32) j) { km = ck[j]; ord = co[j]; c = cc[j]; }
                }
              else { km = __builtin_nontemporal_load (&a.pK[lo + i]); ord = __builtin_nontemporal_load (&a.pT[lo + i]); c = __builtin_nontemporal_load (&a.pC[lo + i]); }
              if (!a.withDepth) c = 0;
              U32 at;
              if (a.slotShift)                                   /* the slot comes with the entry: every entry its own */
                { at = (U32) (km >> MG_SLOT_SHIFT); km &= ((U64) 1 << MG_SLOT_SHIFT) - 1;
                  if (i < nNew) { sKey[at] = km + 1; sOrd[at] = ord; sCnt[at] = c; }
                  else if (c) sCnt[at] += c;
                  continue;
                }
#ifdef MG_ABLATE
              if (a.debug & 32) { at = mgHomeOfM (km, a.g); sKey[at] = km + 1; } else
#endif
              at = mgLdsClaim (sKey, R, mgHomeOfM (km, a.g), km + 1);      /* km: the mixed k-mer the dedup kernel left */
              if (at == R) { a.counters[1] = 1; continue; }
              if (i < nNew) { sOrd[at] = ord; sCnt[at] = c; }
              else if (c) atomicAdd (&sCnt[at], c);
            }
          __syncthreads ();
          for (U32 i0 = 0 ; i0 < R ; i0 += T)
            { const U32 i = i0 + tid;
              unsigned long long k = 0; U32 dep = 0;
              if (i < R)
                { k = sKey[i];
                  uint4 v; v.x = (U32) k; v.y = (U32) (k >> 32); v.z = sOrd[i]; v.w = sCnt[i];
                  { typedef unsigned v4u __attribute__ ((ext_vector_type (4)));
                    v4u vv = { v.x, v.y, v.z, v.w };
                    if (true MG_ABLATE_AND (!(a.debug & 64)))
                    __builtin_nontemporal_store (vv, reinterpret_cast<v4u *> (&a.slots[(U64) b * R + i]));   /* one 16-byte nt store; the 4.3 GB image is not read again this step: keep it out of the caches the rank records live in (2.58 -> 2.53 ms) */
                  }
                  dep = v.w > 0xffffu ? 0xffffu : v.w;
                  if (k) { sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0; }
                }
              if (a.liveHist)                                  /* uniform: depths of a set built by this one add */
                { n1 += (U32) __popcll (__ballot (k && dep == 1));
                  n2 += (U32) __popcll (__ballot (k && dep == 2));
                  if (k && dep != 1 && dep != 2)
                    { if (dep < MG_LIVE_BINS) atomicAdd (&sLive[dep], 1u); else atomicAdd (&a.liveHist[dep], 1ull); }
                }
            }
          __syncthreads ();
          if (tid == 0 && nNew) a.occ[b] += nNew;
        }
      nu = nnu; lo = nlo; occNow = occNext; nNew = nNewNext;
#pragma unroll
      for (int j = 0 ; j < MG_MERGE_PREFETCH ; ++j) { ck[j] = nk[j]; co[j] = no[j]; cc[j] = ncc[j]; }
    }
  if (tid == 0 && sPlaced[0]) { atomicAdd ((unsigned long long *) &a.counters[4], (unsigned long long) sPlaced[0]); if (sPlaced[1]) atomicAdd ((unsigned long long *) &a.counters[5], (unsigned long long) sPlaced[1]); }
  if (a.liveHist)
    { __syncthreads ();
      if ((tid & 63) == 0) { if (n1) atomicAdd (&sLive[1], n1); if (n2) atomicAdd (&sLive[2], n2); }
      __syncthreads ();
      for (U32 i = tid ; i < MG_LIVE_BINS ; i += T) if (sLive[i]) atomicAdd (&a.liveHist[i], (unsigned long long) sLive[i]);
    }
}

/* step 3b: ordinal of the first occurrence -> index, for every new unique of every bucket's list, slice by slice.
 * A wave takes 64 consecutive buckets' group s (one bucket per lane for the bounds, then list by list).  Workgroups
 * b, b + 8, b + 16 ... are placed on one XCD (observed, MI355X_MICROARCH.md; it only matters for speed), and they
 * take the slices x, x + 8, ... one after the other, so an XCD works on one slice at a time and reads its rank records
 * (2^sliceShift / 4 bytes) from its own L2 instead of once per k-mer from the fabric (tools/ubench_rand: 240 G/s
 * against 66 G/s at the whole structure's 39 MB). */
#define MG_LOOKUP_UNROLL 4
__global__ __launch_bounds__ (256)
void mgRankLookupKernel (const MgBucketArgs a, U32 groupsPerSlice)
{
  MG_BUILD_PRIO ();
  const int lane = threadIdx.x & 63;
  const U32 blocksPerSlice = (groupsPerSlice + 3) / 4;
  const U32 xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
  const U32 s = xcd + 8 * (k / blocksPerSlice), g = (k % blocksPerSlice) * 4 + (threadIdx.x >> 6);
  if (s >= a.nSlices || g >= groupsPerSlice) return;
  const U32 b = g * 64 + (U32) lane;
  U64 lo = 0; U32 n = 0;
  if (b < a.nBuckets)
    { const unsigned short *o = a.sliceOff + (U64) b * (a.nSlices + 2) + s;
      const U32 o0 = o[0], o1 = o[1];
      n = o1 - o0; lo = a.bucketStart[b] + o0;
    }
  auto indexOf = [&] (U32 tok, const uint4 &r) -> U32
    { const U64 bits = ((U64) r.y << 32) | r.x;
      const U64 idx = (U64) a.baseMax + 1 + r.z + (U32) __popcll (bits & (((U64) 1 << (tok & 63)) - 1));
      return idx < a.size ? ((U32) idx | MG_ASSIGNED) : 0;
    };
  /* MG_LOOKUP_UNROLL lists per round, all their loads in flight together.  (Fetching the next round's ordinals under
     this round's gathers, or 8 lists per round, changes nothing; nor does using every lane of every gather -- round 6: a wave's 64
     lists flattened, 64 items per instruction instead of a list's 42, 0.935 against 0.897 ms, DESIGN_EXPERIMENTS.md §K: what counts is
     the number of scattered LANES the memory path takes, 115 G/s here, not the number of instructions.) */
  for (int j = 0 ; j < 64 ; j += MG_LOOKUP_UNROLL)
    { U64 l[MG_LOOKUP_UNROLL]; U32 m[MG_LOOKUP_UNROLL], tok[MG_LOOKUP_UNROLL]; uint4 r[MG_LOOKUP_UNROLL];
#pragma unroll
      for (int u = 0 ; u < MG_LOOKUP_UNROLL ; ++u)
        { l[u] = ((U64) (U32) __shfl ((int) (U32) (lo >> 32), j + u) << 32) | (U32) __shfl ((int) (U32) lo, j + u);
          m[u] = (U32) __shfl ((int) n, j + u);
        }
#pragma unroll
      for (int u = 0 ; u < MG_LOOKUP_UNROLL ; ++u)
        { tok[u] = 0; if ((U32) lane < m[u] MG_ABLATE_AND (!(a.debug & 256))) tok[u] = 0x7fffffffu - __builtin_nontemporal_load (&a.pT[l[u] + lane]); }
#pragma unroll
      for (int u = 0 ; u < MG_LOOKUP_UNROLL ; ++u)
        { r[u] = make_uint4 (0, 0, 0, 0); if ((U32) lane < m[u] MG_ABLATE_AND (!(a.debug & 16))) r[u] = *reinterpret_cast<const uint4 *> (&a.grp[tok[u] >> 6]); }
#pragma unroll
      for (int u = 0 ; u < MG_LOOKUP_UNROLL ; ++u) asm volatile ("" : "+v" (r[u].x), "+v" (r[u].y), "+v" (r[u].z));   /* all records in before the first store (see mgRankAssignKernel) */
#pragma unroll
      for (int u = 0 ; u < MG_LOOKUP_UNROLL ; ++u)
        if ((U32) lane < m[u] MG_ABLATE_AND (!(a.debug & 128))) a.pT[l[u] + lane] = indexOf (tok[u], r[u]);
#pragma unroll
      for (int u = 0 ; u < MG_LOOKUP_UNROLL ; ++u)
        for (U32 i = 64 + (U32) lane ; i < m[u] ; i += 64)                /* lists longer than a wave: rare at the usual slice size */
          { const U32 t = 0x7fffffffu - __builtin_nontemporal_load (&a.pT[l[u] + i]);
            const uint4 rr = *reinterpret_cast<const uint4 *> (&a.grp[t >> 6]);
            a.pT[l[u] + i] = indexOf (t, rr);
          }
    }
}

/* the dedup kernel's per-bucket counts of distinct k-mers: out[0] = their sum, out[1] = the largest (out[] zeroed by the launcher) */
__global__ __launch_bounds__ (256)
void mgUniqStatsKernel (const U32 *__restrict__ uniqCount, U32 nBuckets, unsigned long long *__restrict__ out)
{
  unsigned long long sum = 0; U32 mx = 0;
  for (U32 b = blockIdx.x * 256 + threadIdx.x ; b < nBuckets ; b += gridDim.x * 256) { const U32 c = uniqCount[b]; sum += c; mx = c > mx ? c : mx; }
  sum = mgWaveReduce<MgSum> ((U64) sum); mx = mgWaveReduce<MgMax> (mx);
  if ((threadIdx.x & 63) == 0) { if (sum) atomicAdd (&out[0], sum); if (mx) atomicMax (&out[1], (unsigned long long) mx); }
}

/* ======================================================================================== */
/* host side: the launches of mgTableAdd's bucketed leg, in its order                         */

/* A kernel's instance is chosen once (mgForFlag: its template arguments from run-time flags), and what is chosen gets the LDS attribute
   where the launch asks for more than 48 KiB, and is launched. */
MgStatus mgBucketDedup (const MgBucketArgs &a, bool packed, unsigned threads, unsigned grid, U32 perBlock, size_t lds, hipStream_t st)
{
  const U32 R = a.g.R;
  const bool bigR = R > MG_DEDUP_PER * 1024u;       /* R = 8192: the dedup kernel's threads take eight slots each */
  if (R > MG_DEDUP_PER_BIG * 1024u) { mgSetError ("internal: bucket of %u slots", R); return MG_ERR_ARG; }
  if ((U64) threads * (bigR ? MG_DEDUP_PER_BIG : MG_DEDUP_PER) < R)      /* every slot of the image must belong to a thread of the closing sweep */
    { mgSetError ("internal: %u threads for a bucket of %u slots", threads, R); return MG_ERR_ARG; }
  /* oversize buckets first: their chunks reduced to weighted entries by a workgroup each (nothing to do on ordinary data:
     the plan finds no bucket and the reduce kernel's workgroups leave at once) */
  MG_HIP (hipMemsetAsync (a.hotCount, 0, 16, st));
  MG_LAUNCH (MG_K_HOT_REDUCE, st, mgHotPlanKernel, dim3 ((a.nBuckets + 255) / 256), dim3 (256), 0, st, a);
  const size_t ldsHot = (size_t) R * 16 + 16;
  const MgStatus s = mgForFlag (packed, [&] (auto PK) -> MgStatus
    { if (ldsHot > 48 * 1024) MG_HIP (hipFuncSetAttribute ((const void *) mgHotReduceKernel<decltype (PK)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsHot));
      MG_LAUNCH (MG_K_HOT_REDUCE, st, mgHotReduceKernel<decltype (PK)::value>, dim3 (1024), dim3 (threads), ldsHot, st, a);
      return MG_OK;
    });
  if (s) return s;
  return mgForFlag (packed, [&] (auto PK) -> MgStatus { return mgForFlag (a.slotShift != 0, [&] (auto SL) -> MgStatus { return mgForFlag (bigR, [&] (auto BIG) -> MgStatus
    { constexpr bool pk = decltype (PK)::value, sl = decltype (SL)::value;
      constexpr int per = decltype (BIG)::value ? MG_DEDUP_PER_BIG : MG_DEDUP_PER;
      if (lds > 48 * 1024)
        { MG_HIP (hipFuncSetAttribute ((const void *) mgBucketDedupKernel<pk, sl, per, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
          MG_HIP (hipFuncSetAttribute ((const void *) mgBucketDedupKernel<pk, sl, per, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        }
      MG_LAUNCH (MG_K_BUCKET_DEDUP, st, (mgBucketDedupKernel<pk, sl, per, false>), dim3 (grid), dim3 (threads), lds, st, a, perBlock);
      MG_LAUNCH (MG_K_HOT_REDUCE, st, (mgBucketDedupKernel<pk, sl, per, true>), dim3 (64), dim3 (threads), lds, st, a, perBlock);
      return MG_OK;
    }); }); });
}

/* out[0] = the buckets' distinct k-mers, out[1] = the fullest bucket's (two device words, zeroed here) */
MgStatus mgUniqStats (const U32 *uniqCount, U32 nBuckets, unsigned long long *out, hipStream_t st)
{
  const U64 NB = nBuckets;
  MG_HIP (hipMemsetAsync (out, 0, 16, st));
  MG_LAUNCH (MG_K_RANK_SCAN, st, mgUniqStatsKernel, dim3 ((unsigned) (NB / 256 < 256 ? (NB + 255) / 256 : 256)), dim3 (256), 0, st, uniqCount, nBuckets, out);
  return MG_OK;
}

MgStatus mgRankLookup (const MgBucketArgs &a, hipStream_t st)
{
  const U32 groupsPerSlice = (a.nBuckets + 63) / 64;
  const U32 blocksPerSlice = (groupsPerSlice + 3) / 4, rounds = (a.nSlices + 7) / 8;
  MG_LAUNCH (MG_K_RANK_LOOKUP, st, mgRankLookupKernel, dim3 (8 * rounds * blocksPerSlice), dim3 (256), 0, st, a, groupsPerSlice);
  return MG_OK;
}

/* the scan placement keeps a register per unique: the instance that takes only the uniques fetched ahead where no list is longer (the
   tightening has counted the fullest bucket's; otherwise by the bucket's size), the one with MG_PLACE_KEEP otherwise (it spills a little) */
MgStatus mgBucketMerge (const MgBucketArgs &a, U64 fullest, unsigned threads, unsigned grid, U32 perBlock, size_t lds, hipStream_t st)
{
  return mgForFlag (fullest <= (U64) MG_MERGE_PREFETCH * threads, [&] (auto AHEAD) -> MgStatus
    { constexpr int keep = decltype (AHEAD)::value ? MG_MERGE_PREFETCH : MG_PLACE_KEEP;
      if (lds > 48 * 1024) MG_HIP (hipFuncSetAttribute ((const void *) mgBucketMergeKernel<keep>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
      MG_LAUNCH (MG_K_BUCKET_MERGE, st, mgBucketMergeKernel<keep>, dim3 (grid), dim3 (threads), lds, st, a, perBlock);
      return MG_OK;
    });
}
