/* mg_devsort.hip — two device-wide primitives over U32, for whoever has counts to turn into places or values to group by a key: the
 * Reference's pack (mg_refpack.hip: loc[] and rev[] of referencePack, modmap.c:74-91) and the read set's device passes (mg_rsdev.hip:
 * the inverse lists of invBuild, the neighbours of -C and -P).
 *   scan   exclusive sums in tiles of 4096: a sum per tile, the tiles' sums scanned by one workgroup (mgGroupSumKernel), then every tile
 *          scanned from its base;
 *   sort   a STABLE least-significant-digit radix sort, 8 bits a pass.  Stability is what the callers are after: the occurrences of one
 *          modset index stay in occurrence order (queryProcess reads rev[loc[x]] as the FIRST one: modmap.c:219-221,242-254), the reads of
 *          one mod in read order (modasm.c:266,278).  Ranks inside a tile come from wave-level matching (8 ballots give every lane the set
 *          of lanes that hold its digit), so an input that is one key a million times over sorts at the speed of any other.
 * Both get their scratch themselves: a scan its tile words from the caller's MgDevScratch, the sort a histogram that is longer by the tile
 * words of the scans over it -- no caller sizes an array for them.
 */
#include <hip/hip_runtime.h>
#include "mg_prefix.h"
#include "mg_devsort.h"

int mgKeyBits (U64 maxKey)
{ int keyBits = 1; while (keyBits < 32 && ((U64) 1 << keyBits) <= maxKey) ++keyBits; return keyBits; }

/* ---------------------------------------------------------------------------------------- */
/* device-wide exclusive scan of U32                                                          */

__global__ __launch_bounds__ (256)
void mgRefTileSumKernel (const U32 *__restrict__ in, U64 n, U32 *__restrict__ tileSum)
{
  __shared__ U32 lds[4];
  const U64 base = (U64) blockIdx.x * MG_SCAN_TILE;
  U32 s = 0;
  for (int j = 0 ; j < 16 ; ++j) { const U64 i = base + (U64) j * 256 + threadIdx.x; if (i < n) s += in[i]; }
  s = mgBlockReduce<256, MgSum> (s, lds);
  if (!threadIdx.x) tileSum[blockIdx.x] = s;
}
__global__ __launch_bounds__ (256)
void mgRefTileScanKernel (const U32 *__restrict__ in, U64 n, const U32 *__restrict__ tileBase, U32 *__restrict__ out)
{
  __shared__ U32 lds[4];
  const U64 base = (U64) blockIdx.x * MG_SCAN_TILE + (U64) threadIdx.x * 16;      /* a thread's 16 items are consecutive */
  U32 v[16]; U32 s = 0;
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j) { v[j] = base + j < n ? in[base + j] : 0u; s += v[j]; }
  U32 run = tileBase[blockIdx.x] + mgBlockExclusive<256, MgSum> (s, lds);
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j) { if (base + j < n) out[base + j] = run; run += v[j]; }
}

/* a word per tile and the total behind them; rounded up so that it is one expression of n (and what the callers' estimates have always taken) */
size_t mgScanScratchWords (U64 n) { return (size_t) (n / MG_SCAN_TILE) + 4; }

/* the scan over tiles[mgScanScratchWords (n)]; the total is left in tiles[number of tiles] */
static MgStatus mgScanInto (const U32 *in, U32 *out, U64 n, U32 *tiles, hipStream_t st)
{
  const U32 nTiles = (U32) ((n + MG_SCAN_TILE - 1) / MG_SCAN_TILE);
  hipLaunchKernelGGL (mgRefTileSumKernel, dim3 (nTiles), dim3 (256), 0, st, in, n, tiles);
  hipLaunchKernelGGL ((mgGroupSumKernel<U32, U32>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, tiles, tiles, nTiles, tiles + nTiles);
  hipLaunchKernelGGL (mgRefTileScanKernel, dim3 (nTiles), dim3 (256), 0, st, in, n, tiles, out);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

MgStatus mgExclusiveScan (MgDevScratch &scratch, const U32 *in, U32 *out, U64 n, hipStream_t st, U32 *total)
{
  if (total) *total = 0;
  if (!n) return MG_OK;
  U32 *tiles; MgStatus s;
  if ((s = scratch.get (&tiles, mgScanScratchWords (n))) || (s = mgScanInto (in, out, n, tiles, st))) return s;
  if (total && (hipMemcpyAsync (total, tiles + (n + MG_SCAN_TILE - 1) / MG_SCAN_TILE, 4, hipMemcpyDeviceToHost, st) || hipStreamSynchronize (st))) return scratch.fail ();
  return MG_OK;
}

/* ---------------------------------------------------------------------------------------- */
/* one pass of the stable radix sort: a workgroup's tile is 8192 consecutive elements, wave w's part of it elements
   [2048 w, 2048 (w + 1)), taken 64 at a time in order.  hist[digit * nTiles + tile]: digit-major, so that ONE exclusive scan over
   the whole array gives every (digit, tile) its place in the output. */
#define MG_RSORT_WAVE (MG_RSORT_TILE / 4)
__global__ __launch_bounds__ (256)
void mgRefSortHistKernel (const U32 *__restrict__ keys, U64 n, int shift, U32 *__restrict__ hist, U32 nTiles)
{
  __shared__ U32 sC[256];
  sC[threadIdx.x] = 0;
  __syncthreads ();
  const U64 base = (U64) blockIdx.x * MG_RSORT_TILE;
  for (int j = 0 ; j < MG_RSORT_TILE / 256 ; ++j)
    { const U64 i = base + (U64) j * 256 + threadIdx.x;
      if (i < n) atomicAdd (&sC[(keys[i] >> shift) & 255u], 1u);
    }
  __syncthreads ();
  hist[(U64) threadIdx.x * nTiles + blockIdx.x] = sC[threadIdx.x];
}
template <bool FIRST>        /* FIRST: the values are the elements' own positions (the occurrence ordinals) */
__global__ __launch_bounds__ (256)
void mgRefSortScatterKernel (const U32 *__restrict__ keys, const U32 *__restrict__ vals, U64 n, int shift, const U32 *__restrict__ place, U32 nTiles,
                             U32 *__restrict__ keysOut, U32 *__restrict__ valsOut)
{
  __shared__ U32 sC[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int q = 0 ; q < 4 ; ++q) sC[q][threadIdx.x] = 0;
  __syncthreads ();
  const U64 wbase = (U64) blockIdx.x * MG_RSORT_TILE + (U64) w * MG_RSORT_WAVE;
  for (int r = 0 ; r < MG_RSORT_WAVE / 64 ; ++r)
    { const U64 i = wbase + (U64) r * 64 + lane;
      if (i < n) atomicAdd (&sC[w][(keys[i] >> shift) & 255u], 1u);
    }
  __syncthreads ();
  { U32 run = place[(U64) threadIdx.x * nTiles + blockIdx.x];        /* digit threadIdx.x: where the tile's first such element goes; then wave by wave */
    for (int q = 0 ; q < 4 ; ++q) { const U32 c = sC[q][threadIdx.x]; sC[q][threadIdx.x] = run; run += c; }
  }
  __syncthreads ();
  for (int r = 0 ; r < MG_RSORT_WAVE / 64 ; ++r)
    { const U64 i = wbase + (U64) r * 64 + lane;
      const bool live = i < n;
      const U32 key = live ? keys[i] : 0u;
      const U32 dg = (key >> shift) & 255u;
      U64 peers = __ballot (live);                                   /* the lanes that hold my digit */
#pragma unroll
      for (int b = 0 ; b < 8 ; ++b)
        { const U64 m = __ballot ((dg >> b) & 1u);
          peers &= ((dg >> b) & 1u) ? m : ~m;
        }
      const U32 before = (U32) __popcll (peers & (((U64) 1 << lane) - 1));
      const U32 old = sC[w][dg];                                      /* every peer reads the same counter ... */
      __builtin_amdgcn_wave_barrier ();
      if (live && before == 0) sC[w][dg] = old + (U32) __popcll (peers);      /* ... and the first of them moves it on (one wave, LDS in order) */
      __builtin_amdgcn_wave_barrier ();
      if (live)
        { const U32 at = old + before;
          if (keysOut) keysOut[at] = key;
          valsOut[at] = FIRST ? (U32) i : vals[i];
        }
    }
}

MgStatus mgRefStableSort (MgDevScratch &scratch, const U32 *keys, const U32 *vals, U32 n, int keyBits, U32 **out, hipStream_t st)
{
  *out = 0;
  MgDevScratch mine ("stable sort on the device");                   /* what only the passes need goes when they are done */
  const int passes = (keyBits + 7) / 8 > 0 ? (keyBits + 7) / 8 : 1;
  const U32 nSortTiles = (U32) (((U64) n + MG_RSORT_TILE - 1) / MG_RSORT_TILE);
  const size_t histWords = (size_t) 256 * (nSortTiles ? nSortTiles : 1);
  U32 *k1 = 0, *k2 = 0, *v1, *v2, *hist;
  if (mine.get (&hist, histWords + mgScanScratchWords (histWords)) || mine.get (&v1, (size_t) n + 1) || mine.get (&v2, (size_t) n + 1)) return MG_ERR_HIP;
  if (passes > 1 && (mine.get (&k1, n) || (passes > 2 && mine.get (&k2, n)))) return MG_ERR_HIP;
  const U32 *kin = keys; const U32 *vin = vals;
  U32 *kout = k1, *vout = v1;
  for (int p = 0 ; p < passes ; ++p)
    { const bool last = p + 1 == passes;
      hipLaunchKernelGGL (mgRefSortHistKernel, dim3 (nSortTiles), dim3 (256), 0, st, kin, (U64) n, 8 * p, hist, nSortTiles);
      MgStatus s = mgScanInto (hist, hist, histWords, hist + histWords, st);
      if (s) return s;
      if (!vin) hipLaunchKernelGGL (mgRefSortScatterKernel<true>, dim3 (nSortTiles), dim3 (256), 0, st, kin, vin, (U64) n, 8 * p, hist, nSortTiles, last ? (U32 *) 0 : kout, vout);
      else hipLaunchKernelGGL (mgRefSortScatterKernel<false>, dim3 (nSortTiles), dim3 (256), 0, st, kin, vin, (U64) n, 8 * p, hist, nSortTiles, last ? (U32 *) 0 : kout, vout);
      kin = kout; vin = vout;
      kout = kout == k1 ? k2 : k1; vout = vout == v1 ? v2 : v1;
    }
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st) != hipSuccess) return mine.fail ();
  scratch.adopt (*out = mine.take ((U32 *) vin));                        /* the last pass's output */
  return MG_OK;
}
