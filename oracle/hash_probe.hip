/* oracle/hash_probe.hip — TEST INFRASTRUCTURE ONLY.
 *
 * libhashprobe.so: the device arithmetic of modimizer_amd/csrc/mg_common.h -- the scan's hit tests (mgDivisible, mgDivisibleOdd,
 * mgDivisibleOdd32, mgDivisibleAny32), the reverse complements (mgRevComp16, mgRevComp) and the table's hash (mgMixBits, mgMixK,
 * mgMixTopOfKmer, mgBucketOfM, mgHomeOfM) -- behind plain entry points, so that tests/test_gpu_hashprobe.py can hold each against
 * integer arithmetic on values of its own choosing: every odd modulus below 2^15 at 40-bit hashes, multiples next to 2^24 j, 2^32 and
 * 2^(2k), every width of the mix.  The scan reaches them only with the hashes a batch happens to hold, where a wrong answer once in
 * d 10^6 is invisible.
 *
 * The kernels here are trivial: grid-stride, one element per thread, a call of the header's function and a store.  The functions are
 * __forceinline__ in a header, so what runs is this file's compile of them, with the header's hash baked in (below).  MgHashParams is
 * NOT made here: the probe is LINKED against modimizer_amd/libmodgpu.so and calls the library's own mgMakeParams on a Seqhash
 * {k, w = d, shift1, mask, factor1} it fabricates from its arguments.
 *
 * Every entry point takes HOST pointers and works on the null stream: it allocates, copies in, launches, copies back, frees, and
 * returns 0, the MgStatus, or -1 (refused: what the library would never run that function on).  The Makefile bakes a hash of this
 * file and mg_common.h into it (hash_probe.inc); hashProbeHash () returns it and the tests compare it with the tree's. */
#include <string.h>
#include "../modimizer_amd/csrc/mg_common.h"
#include "hash_probe.inc"

static const char gProbeMarker[] = "HASH_PROBE_HASH=" HASH_PROBE_HASH;
extern "C" const char *hashProbeHash (void) { return gProbeMarker + 16; }

#define PROBE_HIP(call) do { if ((call) != hipSuccess) return (int) scratch.fail (); } while (0)
#define PROBE_THREADS 256

enum { HP_ANY64 = 0, HP_ODD64, HP_ODD32, HP_ANY32, HP_DIV_COUNT };
enum { HP_MIX_BITS = 0, HP_MIX_K, HP_MIX_TOP, HP_MIX_BUCKET, HP_MIX_HOME, HP_MIX_COUNT };

/* the library's parameters of a hasher (k, d): false when there is no such hasher */
static bool probeParams (int k, U32 d, MgHashParams *p)
{
  if (k < 1 || k > 31 || d < 1) return false;
  Seqhash sh; memset (&sh, 0, sizeof (sh));
  sh.k = k; sh.w = (int) d; sh.shift1 = 64 - 2 * k; sh.shift2 = 2 * k - 1;
  sh.mask = ((U64) 1 << (2 * k)) - 1;
  sh.factor1 = 0x9E3779B97F4A7C15ull;            /* any odd number: no function under test reads it */
  *p = mgMakeParams (&sh);
  return true;
}

/* out12: factor1, mask, k, shift1, d, dShift, dOddInv, dOddLim, c24, inv32, lim32, small32 */
extern "C" int hashProbeParams (int k, U32 d, U64 *out12)
{
  MgHashParams p;
  if (!probeParams (k, d, &p)) return -1;
  out12[0] = p.factor1; out12[1] = p.mask; out12[2] = (U64) p.k; out12[3] = (U64) p.shift1; out12[4] = p.d; out12[5] = (U64) p.dShift;
  out12[6] = p.dOddInv; out12[7] = p.dOddLim; out12[8] = p.c24; out12[9] = p.inv32; out12[10] = p.lim32; out12[11] = p.small32;
  return 0;
}

/* element i is tested against modulus i / per: out[i] = 1 when h[i] is a multiple of it */
template <int WHICH>
__global__ void __launch_bounds__ (PROBE_THREADS) hashProbeDivKernel (const MgHashParams *params, const U64 *h, U64 n, U64 per, U8 *out)
{
  for (U64 i = (U64) blockIdx.x * PROBE_THREADS + threadIdx.x ; i < n ; i += (U64) gridDim.x * PROBE_THREADS)
    { const MgHashParams p = params[i / per];
      bool hit;
      if (WHICH == HP_ANY64)      hit = mgDivisible (h[i], p);
      else if (WHICH == HP_ODD64) hit = mgDivisibleOdd (h[i], p);
      else if (WHICH == HP_ODD32) hit = mgDivisibleOdd32 (h[i], p);
      else                        hit = mgDivisibleAny32 (h[i], p);
      out[i] = hit ? 1 : 0;
    }
}

/* nD moduli, per values of h for each (h[m * per + j] belongs to d[m]), ONE launch.  Refused (-1): a modulus the library would never
 * give to that function -- the 32-bit tests where small32 == 0 (and h of 2^40 or more), the odd tests where d is even */
extern "C" int hashProbeDivisibleMany (int which, int k, const U32 *d, U64 nD, const U64 *h, U64 per, U8 *out)
{
  if (which < 0 || which >= HP_DIV_COUNT || !nD || !per || nD > ((U64) 1 << 20) || per > ((U64) 1 << 24) || nD * per > ((U64) 1 << 28)) return -1;
  std::vector<MgHashParams> params ((size_t) nD);
  for (U64 m = 0 ; m < nD ; ++m)
    { MgHashParams &p = params[(size_t) m];
      if (!probeParams (k, d[m], &p)) return -1;
      if ((which == HP_ODD32 || which == HP_ANY32) && !p.small32) return -1;
      if ((which == HP_ODD64 || which == HP_ODD32) && p.dShift != 0) return -1;
    }
  const U64 n = nD * per;
  if (which == HP_ODD32 || which == HP_ANY32)
    for (U64 i = 0 ; i < n ; ++i) if (h[i] >> 40) return -1;
  MgDevScratch scratch ("hash probe: divisible");
  MgHashParams *dParams; U64 *dH; U8 *dOut;
  if (scratch.get (&dParams, (size_t) nD) || scratch.get (&dH, (size_t) n) || scratch.get (&dOut, (size_t) n)) return (int) MG_ERR_HIP;
  PROBE_HIP (hipMemcpy (dParams, params.data (), (size_t) nD * sizeof (MgHashParams), hipMemcpyHostToDevice));
  PROBE_HIP (hipMemcpy (dH, h, (size_t) n * 8, hipMemcpyHostToDevice));
  PROBE_HIP (hipMemset (dOut, 0xEE, (size_t) n));
  const dim3 grid (mgGrid (n, PROBE_THREADS)), block (PROBE_THREADS);
  if (which == HP_ANY64)      hipLaunchKernelGGL (hashProbeDivKernel<HP_ANY64>, grid, block, 0, 0, dParams, dH, n, per, dOut);
  else if (which == HP_ODD64) hipLaunchKernelGGL (hashProbeDivKernel<HP_ODD64>, grid, block, 0, 0, dParams, dH, n, per, dOut);
  else if (which == HP_ODD32) hipLaunchKernelGGL (hashProbeDivKernel<HP_ODD32>, grid, block, 0, 0, dParams, dH, n, per, dOut);
  else                        hipLaunchKernelGGL (hashProbeDivKernel<HP_ANY32>, grid, block, 0, 0, dParams, dH, n, per, dOut);
  PROBE_HIP (hipGetLastError ());
  PROBE_HIP (hipMemcpy (out, dOut, (size_t) n, hipMemcpyDeviceToHost));
  return 0;
}

/* one modulus: out[i] = 1 when h[i] is a multiple of d */
extern "C" int hashProbeDivisible (int which, int k, U32 d, const U64 *h, U64 n, U8 *out)
{ return hashProbeDivisibleMany (which, k, &d, 1, h, n, out); }

__global__ void __launch_bounds__ (PROBE_THREADS) hashProbeRevComp16Kernel (const U32 *x, U64 n, U32 *out)
{
  for (U64 i = (U64) blockIdx.x * PROBE_THREADS + threadIdx.x ; i < n ; i += (U64) gridDim.x * PROBE_THREADS) out[i] = mgRevComp16 (x[i]);
}

__global__ void __launch_bounds__ (PROBE_THREADS) hashProbeRevCompKernel (const U64 *x, U64 n, int shift1, U64 *out)
{
  for (U64 i = (U64) blockIdx.x * PROBE_THREADS + threadIdx.x ; i < n ; i += (U64) gridDim.x * PROBE_THREADS) out[i] = mgRevComp (x[i], shift1);
}

/* words of 16 bases, the first base on top */
extern "C" int hashProbeRevComp16 (const U32 *x, U64 n, U32 *out)
{
  if (!n || n > ((U64) 1 << 28)) return -1;
  MgDevScratch scratch ("hash probe: revcomp16");
  U32 *dX, *dOut;
  if (scratch.get (&dX, (size_t) n) || scratch.get (&dOut, (size_t) n)) return (int) MG_ERR_HIP;
  PROBE_HIP (hipMemcpy (dX, x, (size_t) n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL (hashProbeRevComp16Kernel, dim3 (mgGrid (n, PROBE_THREADS)), dim3 (PROBE_THREADS), 0, 0, dX, n, dOut);
  PROBE_HIP (hipGetLastError ());
  PROBE_HIP (hipMemcpy (out, dOut, (size_t) n * 4, hipMemcpyDeviceToHost));
  return 0;
}

/* k-mers in the low 2k bits (refused: a value with bits above them, as the scan never makes one) */
extern "C" int hashProbeRevComp (int k, const U64 *x, U64 n, U64 *out)
{
  if (k < 1 || k > 31 || !n || n > ((U64) 1 << 28)) return -1;
  for (U64 i = 0 ; i < n ; ++i) if (x[i] >> (2 * k)) return -1;
  MgDevScratch scratch ("hash probe: revcomp");
  U64 *dX, *dOut;
  if (scratch.get (&dX, (size_t) n) || scratch.get (&dOut, (size_t) n)) return (int) MG_ERR_HIP;
  PROBE_HIP (hipMemcpy (dX, x, (size_t) n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL (hashProbeRevCompKernel, dim3 (mgGrid (n, PROBE_THREADS)), dim3 (PROBE_THREADS), 0, 0, dX, n, 64 - 2 * k, dOut);
  PROBE_HIP (hipGetLastError ());
  PROBE_HIP (hipMemcpy (out, dOut, (size_t) n * 8, hipMemcpyDeviceToHost));
  return 0;
}

/* b and arg are kernel arguments, not template ones: the library's kernels take the width from a struct at run time too */
__global__ void __launch_bounds__ (PROBE_THREADS) hashProbeMixKernel (int what, int b, U32 arg, const U64 *x, U64 n, U64 *out)
{
  MgGeom g; g.kbits = b; g.log2NB = what == HP_MIX_BUCKET ? (int) arg : 0; g.R = what == HP_MIX_HOME ? arg : 64u;
  for (U64 i = (U64) blockIdx.x * PROBE_THREADS + threadIdx.x ; i < n ; i += (U64) gridDim.x * PROBE_THREADS)
    { const U64 v = x[i];
      U64 r;
      if (what == HP_MIX_BITS)        r = mgMixBits (v, b);
      else if (what == HP_MIX_K)      r = mgMixK (v, b);
      else if (what == HP_MIX_TOP)    r = mgMixTopOfKmer (v, b, (int) arg);
      else if (what == HP_MIX_BUCKET) r = mgBucketOfM (mgMixK (v, b), g);
      else                            r = mgHomeOfM (mgMixK (v, b), g);
      out[i] = r;
    }
}

/* x: b-bit values (k-mers of b / 2 bases).  bits: mgMixBits (x, b); k: mgMixK (x, b); top: mgMixTopOfKmer (x, b, hiB = arg), b >= 24 and
 * 1 <= hiB <= MG_MIX_TOP; bucket: mgBucketOfM of the k-mer's mix in a table of 2^arg buckets; home: mgHomeOfM of it in a bucket of
 * R = arg slots */
extern "C" int hashProbeMix (int what, int b, U32 arg, const U64 *x, U64 n, U64 *out)
{
  if (what < 0 || what >= HP_MIX_COUNT || b < 1 || b > 62 || !n || n > ((U64) 1 << 28)) return -1;
  if (what == HP_MIX_TOP && (b < 24 || arg < 1 || arg > MG_MIX_TOP)) return -1;
  if (what == HP_MIX_BUCKET && arg > 30) return -1;
  if (what == HP_MIX_HOME && !arg) return -1;
  for (U64 i = 0 ; i < n ; ++i) if (x[i] >> b) return -1;
  MgDevScratch scratch ("hash probe: mix");
  U64 *dX, *dOut;
  if (scratch.get (&dX, (size_t) n) || scratch.get (&dOut, (size_t) n)) return (int) MG_ERR_HIP;
  PROBE_HIP (hipMemcpy (dX, x, (size_t) n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL (hashProbeMixKernel, dim3 (mgGrid (n, PROBE_THREADS)), dim3 (PROBE_THREADS), 0, 0, what, b, arg, dX, n, dOut);
  PROBE_HIP (hipGetLastError ());
  PROBE_HIP (hipMemcpy (out, dOut, (size_t) n * 8, hipMemcpyDeviceToHost));
  return 0;
}
