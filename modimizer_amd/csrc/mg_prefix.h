/* mg_prefix.h — the integer prefix scans and reductions of the library's kernels, written once: over a wave, over a workgroup, and over
 * n counts by one workgroup of 1024.  Two operations, sum and max, over U32 or U64; 0 is the identity of both.
 *
 * What is NOT here, on purpose: mgSegScanKernel (mg_scan.hip: its staged, padded layout was measured, and it is on config 2's step);
 * mgPartScanKernel (mg_part.hip: one count per thread, no pieces); MG_MAX_DPP / mgWavePrefixMax and the merge kernel's prefix-scan
 * placement (mg_bucket.hip); the arg-min over a struct in mg_minimizer.hip; the ballot / popcount placement of mgRsWriteKernel and
 * mgRefAppendKernel.  These are other patterns. */
#ifndef MG_PREFIX_H
#define MG_PREFIX_H
#include <type_traits>
#include "mg_common.h"

#define MG_GROUP_THREADS 1024      /* the workgroup of mgGroupScan */

struct MgSum { template <class T> static __device__ __forceinline__ T op (T a, T b) { return a + b; } };
struct MgMax { template <class T> static __device__ __forceinline__ T op (T a, T b) { return b > a ? b : a; } };

/* ---- wave ------------------------------------------------------------------------------ */

/* inclusive prefix sum over the 64 lanes of a wave with DPP only (no LDS traffic): Hillis-Steele inside the
 * rows of 16 (row_shr 1,2,4,8), then lane 15 of rows 0 and 2 into rows 1 and 3 (row_bcast:15), then lane 31
 * into rows 2 and 3 (row_bcast:31).  Lanes without a source add 0. */
__device__ __forceinline__ U32 mgWaveInclusiveSum (U32 v)
{
  v += (U32) __builtin_amdgcn_update_dpp (0, (int) v, 0x111, 0xf, 0xf, false);
  v += (U32) __builtin_amdgcn_update_dpp (0, (int) v, 0x112, 0xf, 0xf, false);
  v += (U32) __builtin_amdgcn_update_dpp (0, (int) v, 0x114, 0xf, 0xf, false);
  v += (U32) __builtin_amdgcn_update_dpp (0, (int) v, 0x118, 0xf, 0xf, false);
  v += (U32) __builtin_amdgcn_update_dpp (0, (int) v, 0x142, 0xa, 0xf, false);
  v += (U32) __builtin_amdgcn_update_dpp (0, (int) v, 0x143, 0xc, 0xf, false);
  return v;
}
/* the value of the lane off below / of the lane whose number differs in the bits of off (a U64 goes as two words) */
__device__ __forceinline__ U32 mgLaneUp (U32 v, int off) { return (U32) __shfl_up ((int) v, off); }
__device__ __forceinline__ U64 mgLaneUp (U64 v, int off) { return ((U64) mgLaneUp ((U32) (v >> 32), off) << 32) | mgLaneUp ((U32) v, off); }
__device__ __forceinline__ U32 mgLaneXor (U32 v, int off) { return (U32) __shfl_xor ((int) v, off); }
__device__ __forceinline__ U64 mgLaneXor (U64 v, int off) { return ((U64) mgLaneXor ((U32) (v >> 32), off) << 32) | mgLaneXor ((U32) v, off); }

/* every lane gets the wave's sum / max */
template <class Op, class T> __device__ __forceinline__ T mgWaveReduce (T v)
{
  for (int off = 32 ; off ; off >>= 1) v = Op::op (v, mgLaneXor (v, off));
  return v;
}
/* lane l gets v(0) op ... op v(l) */
template <class Op, class T> __device__ __forceinline__ T mgWaveInclusive (T v)
{
  if constexpr (std::is_same<Op, MgSum>::value && std::is_same<T, U32>::value) return mgWaveInclusiveSum (v);
  else
    { const int lane = threadIdx.x & 63;
      for (int off = 1 ; off < 64 ; off <<= 1) { const T o = mgLaneUp (v, off); if (lane >= off) v = Op::op (v, o); }
      return v;
    }
}

/* ---- workgroup of THREADS (a multiple of 64; every thread calls) -------------------------
 * lds: THREADS / 64 words from the caller, free again on return; two barriers. */

/* every thread gets the workgroup's sum / max */
template <int THREADS, class Op, class T> __device__ __forceinline__ T mgBlockReduce (T v, T *lds)
{
  static_assert (THREADS % 64 == 0, "whole waves");
  v = mgWaveReduce<Op> (v);
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads ();
  T tot = 0;
  #pragma unroll
  for (U32 i = 0 ; i < THREADS / 64 ; ++i) tot = Op::op (tot, lds[i]);
  __syncthreads ();
  return tot;
}
/* from the waves' inclusive values: what the waves before this thread's hold together; *total = the workgroup's */
template <int THREADS, class Op, class T> __device__ __forceinline__ T mgBlockBefore (T waveInc, T *lds, T *total)
{
  static_assert (THREADS % 64 == 0, "whole waves");
  const U32 wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 63u) lds[wv] = waveInc;
  __syncthreads ();
  T before = 0, tot = 0;
  #pragma unroll
  for (U32 i = 0 ; i < THREADS / 64 ; ++i) { const T s = lds[i]; before = Op::op (before, i < wv ? s : (T) 0); tot = Op::op (tot, s); }
  __syncthreads ();
  *total = tot;
  return before;
}
/* thread t gets v(0) op ... op v(t) */
template <int THREADS, class Op, class T> __device__ __forceinline__ T mgBlockInclusive (T v, T *lds, T *total)
{
  const T inc = mgWaveInclusive<Op> (v);
  return Op::op (mgBlockBefore<THREADS, Op> (inc, lds, total), inc);
}
/* thread t gets v(0) op ... op v(t - 1), thread 0 gets 0: the inclusive value less the thread's own for a sum, that of the thread before for a max */
template <int THREADS, class Op, class T> __device__ __forceinline__ T mgBlockExclusive (T v, T *lds)
{
  T total;
  const T inc = mgWaveInclusive<Op> (v);
  const T before = mgBlockBefore<THREADS, Op> (inc, lds, &total);
  if constexpr (std::is_same<Op, MgSum>::value) return before + inc - v;
  else { const T up = mgLaneUp (inc, 1); return Op::op (before, (threadIdx.x & 63u) ? up : (T) 0); }
}

/* ---- one workgroup of MG_GROUP_THREADS, n counts -----------------------------------------
 * out[i] = carryIn op in[0] op ... op in[i - 1] for i < n; every thread returns carryIn op in[0] op ... op in[n - 1].  in == out is allowed,
 * and TO may be wider than TI.  Thread t takes the ceil (n / 1024) counts from t * that on (none, if they start at n or beyond), the
 * threads' values are scanned by Hillis-Steele over lds (1024 words, free again on return).  N: the width of n and of the index arithmetic.
 * Precondition: n + 1023 and lo + per (at most n + per - 1, per <= n / 1024 + 1) must not overflow N.  Every present caller holds n far below
 * that: n is a number of tiles, blocks or reads of one batch. */
template <class Op, class TI, class TO, class N> __device__ __forceinline__ TO mgGroupScan (const TI *in, TO *out, N n, TO carryIn, TO *lds)
{
  const U32 tid = threadIdx.x;
  const N per = (n + (MG_GROUP_THREADS - 1)) / MG_GROUP_THREADS;
  const N lo = (N) tid * per < n ? (N) tid * per : n, hi = lo + per < n ? lo + per : n;
  TO acc = 0;
  for (N i = lo ; i < hi ; ++i) acc = Op::op (acc, (TO) in[i]);
  lds[tid] = acc;
  __syncthreads ();
  for (U32 off = 1 ; off < MG_GROUP_THREADS ; off <<= 1)
    { const TO o = tid >= off ? lds[tid - off] : (TO) 0;
      __syncthreads ();
      lds[tid] = Op::op (lds[tid], o);
      __syncthreads ();
    }
  TO run = Op::op (carryIn, tid ? lds[tid - 1] : (TO) 0);
  const TO all = Op::op (carryIn, lds[MG_GROUP_THREADS - 1]);
  __syncthreads ();
  for (N i = lo ; i < hi ; ++i) { const TO x = (TO) in[i]; out[i] = run; run = Op::op (run, x); }
  return all;
}

/* the plain case as a kernel: out[] = the exclusive sums of in[0 .. n), *total = their sum (out + n, or a counter) */
template <class TI, class TO> __global__ __launch_bounds__ (MG_GROUP_THREADS) void mgGroupSumKernel (const TI *in, TO *out, U32 n, TO *total)
{
  __shared__ TO lds[MG_GROUP_THREADS];
  const TO all = mgGroupScan<MgSum> (in, out, n, (TO) 0, lds);
  if (threadIdx.x == 0) *total = all;
}
#endif
