/* oracle/prefix_probe.hip — TEST INFRASTRUCTURE ONLY.
 *
 * libprefixprobe.so: the scans and reductions of modimizer_amd/csrc/mg_prefix.h behind plain entry points, so that
 * tests/test_gpu_prefix.py can hold each of them against numpy on inputs of its own choosing (carries across bit 32, values that
 * differ in the high word only, sums that wrap, a maximum in a given lane, a carry into a max, n around the multiples of 1024).
 * The library's kernels reach the header only with what their data happens to be.
 *
 * Every entry point takes HOST pointers: it allocates, copies in, launches, synchronises, copies back, frees, and returns the
 * hipError_t as an int (-1: no such instantiation).  The tests load this library after libmodgpu.so, so the process holds one HIP
 * runtime.  The Makefile bakes a hash of this file and of mg_prefix.h into it (prefix_probe.inc); prefixProbeHash () returns it and
 * the tests compare it with the tree's: a probe built from other sources cannot pass. */
#include <string.h>
#include "../modimizer_amd/csrc/mg_prefix.h"
#include "prefix_probe.inc"

static const char gProbeMarker[] = "PREFIX_PROBE_HASH=" PREFIX_PROBE_HASH;
extern "C" const char *prefixProbeHash (void) { return gProbeMarker + 18; }

/* ---- wave and workgroup ------------------------------------------------------------------
 * A grid of PROBE_GROUPS workgroups of THREADS; thread g = blockIdx.x * THREADS + threadIdx.x reads in[g].  The five calls follow each
 * other on ONE lds array, as the parsers make them (mg_textgpu.hip).  out: six planes of PROBE_GROUPS * THREADS values:
 * block inclusive, its *total, block exclusive, block reduce, wave inclusive, wave reduce. */
#define PROBE_GROUPS 3
#define PROBE_PLANES 6

template <int THREADS, class Op, class T> __global__ __launch_bounds__ (THREADS) void probeBlockKernel (const T *__restrict__ in, T *__restrict__ out)
{
  __shared__ T lds[THREADS / 64];
  const U32 g = blockIdx.x * THREADS + threadIdx.x, n = PROBE_GROUPS * THREADS;
  const T v = in[g];
  T total;
  const T inc = mgBlockInclusive<THREADS, Op> (v, lds, &total);
  const T exc = mgBlockExclusive<THREADS, Op> (v, lds);
  const T red = mgBlockReduce<THREADS, Op> (v, lds);
  const T wInc = mgWaveInclusive<Op> (v);
  const T wRed = mgWaveReduce<Op> (v);
  out[g] = inc; out[n + g] = total; out[2 * n + g] = exc; out[3 * n + g] = red; out[4 * n + g] = wInc; out[5 * n + g] = wRed;
}

template <int THREADS, class Op, class T> static int probeBlockRun (const void *hIn, void *hOut)
{
  const size_t n = (size_t) PROBE_GROUPS * THREADS;
  T *dIn = 0, *dOut = 0;
  hipError_t e;
  do {
    if ((e = hipMalloc ((void **) &dIn, n * sizeof (T))) || (e = hipMalloc ((void **) &dOut, PROBE_PLANES * n * sizeof (T)))) break;
    if ((e = hipMemcpy (dIn, hIn, n * sizeof (T), hipMemcpyHostToDevice)) || (e = hipMemset (dOut, 0xa5, PROBE_PLANES * n * sizeof (T)))) break;
    hipLaunchKernelGGL ((probeBlockKernel<THREADS, Op, T>), dim3 (PROBE_GROUPS), dim3 (THREADS), 0, 0, dIn, dOut);
    if ((e = hipGetLastError ()) || (e = hipDeviceSynchronize ())) break;
    e = hipMemcpy (hOut, dOut, PROBE_PLANES * n * sizeof (T), hipMemcpyDeviceToHost);
  } while (0);
  (void) hipFree (dIn); (void) hipFree (dOut);
  return (int) e;
}

template <class Op, class T> static int probeBlockThreads (int threads, const void *hIn, void *hOut)
{
  switch (threads)
    { case 64: return probeBlockRun<64, Op, T> (hIn, hOut);
      case 256: return probeBlockRun<256, Op, T> (hIn, hOut);
      case 1024: return probeBlockRun<1024, Op, T> (hIn, hOut);
    }
  return -1;
}

/* threads: 64, 256 or 1024; op: "sum" or "max"; bits: 32 or 64.  in: 3 * threads values, out: 6 planes of as many */
extern "C" int prefixProbeBlock (int threads, const char *op, int bits, const void *in, void *out)
{
  const bool sum = !strcmp (op, "sum");
  if (!sum && strcmp (op, "max")) return -1;
  if (bits == 32) return sum ? probeBlockThreads<MgSum, U32> (threads, in, out) : probeBlockThreads<MgMax, U32> (threads, in, out);
  if (bits == 64) return sum ? probeBlockThreads<MgSum, U64> (threads, in, out) : probeBlockThreads<MgMax, U64> (threads, in, out);
  return -1;
}

/* ---- one workgroup of MG_GROUP_THREADS, n counts ------------------------------------------ */

template <class Op, class TI, class TO, class N> __global__ __launch_bounds__ (MG_GROUP_THREADS) void probeGroupKernel (const TI *in, TO *out, N n, TO carryIn, TO *ret)
{
  __shared__ TO lds[MG_GROUP_THREADS];
  const TO all = mgGroupScan<Op, TI, TO, N> (in, out, n, carryIn, lds);
  if (threadIdx.x == 0) *ret = all;
}

/* hIn: n values of TI, copied back after the launch (the test checks that they are what they were).  hOut: guard + n + guard values
 * of TO; the whole of it goes up before the launch and comes back after it, the kernel's out[] being the n in the middle.  inPlace
 * (TI == TO only): in[] IS out[], so the middle of hOut holds the input and hIn is not used.  *hRet: what thread 0 wrote into a word
 * of its own (0xa5 in every byte if nothing was written). */
template <class TI, class TO, class Launch> static int probeGroupRun (void *hIn, void *hOut, U64 n, U64 guard, int inPlace, U64 *hRet, Launch launch)
{
  if (inPlace && sizeof (TI) != sizeof (TO)) return -1;
  const size_t inBytes = (size_t) n * sizeof (TI), outBytes = (size_t) (n + 2 * guard) * sizeof (TO);
  TI *dIn = 0; TO *dOut = 0, *dRet = 0, ret = 0;
  hipError_t e;
  do {
    if ((e = hipMalloc ((void **) &dIn, inBytes + 16)) || (e = hipMalloc ((void **) &dOut, outBytes + 16)) || (e = hipMalloc ((void **) &dRet, 16))) break;
    if (!inPlace && inBytes && (e = hipMemcpy (dIn, hIn, inBytes, hipMemcpyHostToDevice))) break;
    if (outBytes && (e = hipMemcpy (dOut, hOut, outBytes, hipMemcpyHostToDevice))) break;
    if ((e = hipMemset (dRet, 0xa5, 16))) break;
    launch (inPlace ? (const TI *) (dOut + guard) : (const TI *) dIn, dOut + guard, dRet);
    if ((e = hipGetLastError ()) || (e = hipDeviceSynchronize ())) break;
    if (!inPlace && inBytes && (e = hipMemcpy (hIn, dIn, inBytes, hipMemcpyDeviceToHost))) break;
    if (outBytes && (e = hipMemcpy (hOut, dOut, outBytes, hipMemcpyDeviceToHost))) break;
    if ((e = hipMemcpy (&ret, dRet, sizeof (TO), hipMemcpyDeviceToHost))) break;
    *hRet = (U64) ret;
  } while (0);
  (void) hipFree (dIn); (void) hipFree (dOut); (void) hipFree (dRet);
  return (int) e;
}

template <class Op, class TI, class TO, class N> static int probeGroupScan (void *hIn, void *hOut, U64 n, U64 carryIn, U64 guard, int inPlace, U64 *hRet)
{
  return probeGroupRun<TI, TO> (hIn, hOut, n, guard, inPlace, hRet, [=] (const TI *in, TO *out, TO *ret)
    { hipLaunchKernelGGL ((probeGroupKernel<Op, TI, TO, N>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, 0, in, out, (N) n, (TO) carryIn, ret); });
}
/* mgGroupSumKernel itself: no carry, the total into the word of its own */
template <class TI, class TO> static int probeGroupSum (void *hIn, void *hOut, U64 n, U64 carryIn, U64 guard, int inPlace, U64 *hRet)
{
  if (carryIn) return -1;
  return probeGroupRun<TI, TO> (hIn, hOut, n, guard, inPlace, hRet, [=] (const TI *in, TO *out, TO *ret)
    { hipLaunchKernelGGL ((mgGroupSumKernel<TI, TO>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, 0, in, out, (U32) n, ret); });
}

/* what: "<op>_<in bits>_<out bits>_n<bits of n>" for mgGroupScan<Op, TI, TO, N>, "kernel_<in bits>_<out bits>" for mgGroupSumKernel<TI, TO> */
extern "C" int prefixProbeGroup (const char *what, void *in, void *out, U64 n, U64 carryIn, U64 guard, int inPlace, U64 *ret)
{
  static const struct { const char *name; int (*run) (void *, void *, U64, U64, U64, int, U64 *); } table[] = {
    { "sum_32_32_n32", probeGroupScan<MgSum, U32, U32, U32> }, { "sum_32_64_n32", probeGroupScan<MgSum, U32, U64, U32> },
    { "sum_32_64_n64", probeGroupScan<MgSum, U32, U64, U64> }, { "sum_64_64_n32", probeGroupScan<MgSum, U64, U64, U32> },
    { "sum_64_64_n64", probeGroupScan<MgSum, U64, U64, U64> }, { "max_32_32_n32", probeGroupScan<MgMax, U32, U32, U32> },
    { "max_64_64_n64", probeGroupScan<MgMax, U64, U64, U64> },
    { "kernel_32_32", probeGroupSum<U32, U32> }, { "kernel_32_64", probeGroupSum<U32, U64> }, { "kernel_64_64", probeGroupSum<U64, U64> },
  };
  if (n >= ((U64) 1 << 31)) return -1;
  for (size_t i = 0 ; i < sizeof (table) / sizeof (table[0]) ; ++i)
    if (!strcmp (what, table[i].name)) return table[i].run (in, out, n, carryIn, guard, inPlace, ret);
  return -1;
}
