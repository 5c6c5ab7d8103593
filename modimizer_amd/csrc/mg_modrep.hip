/* mg_modrep.hip — modrep -R <ref.fa> <ref.mod> -s3 <reads.fa> <reads.mod> on the device (modrep.c:27-63,170-268).
 *
 * -R (refCreate): the one reference sequence is scanned and looked up in its set; a lane per hit scatters (loc, strand) packed into one
 * word with atomicMax, so the LAST occurrence of an entry wins (modrep.c:49-50 in scan order), and takes the smallest non-zero loc per
 * entry with atomicMin: the program dies at the first hit whose entry already has a non-zero pos (modrep.c:48), which is the smallest
 * loc that lies above its entry's smallest non-zero one.
 *
 * -s3 (analyzeSequences3), per batch:
 *   vote     scan with the reference set's hasher, lookups in the reference set; the found hits are ranked inside their read by an
 *            exclusive scan of the found flags minus its value at the read's first modimizer (the scan's output is in (read, pos) order);
 *            ranks below 100 add to the read's seqF / seqR with integer atomics (counts: order free); a lane per read writes the verdict;
 *   orient   the good reads are compacted (exclusive scan of the good flags, then of their lengths) and written into a second packed
 *            array, the flipped ones reverse-complemented (3 - base, reversed: modrep.c:215-220); that batch is scanned by the same kernel;
 *   hits     lookups in the second set; the found ones are compacted in order behind the run's hits so far: (k, x, good read ordinal).
 * At the end of the file the hits' ordinals are sorted stably by k (mgRefStableSort): inside a mod they stay in read order, so the
 * occurrences of a mod in ONE read are neighbours -- what the program finds with an array of ms->max bytes that it clears per read
 * (modrep.c:225,229).  One pass adds n[k] and nPre[k]; the counts, the zeroing, the per-read maximum and the "minimum max" fold follow.
 * The hits stay on the device between batches (MgDevBuf); what a call needs besides them is its MgDevScratch's.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <vector>
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_devsort.h"
#include "mg_modrep_int.h"

#define MG_REP_VOTES 100u         /* modrep.c:197,204 */
#define MG_REP_MIXED 10u          /* modrep.c:204 */

static thread_local int gRepPath = -1;
extern "C" int mgRepPath (void) { return gRepPath; }
void mgRepPathSet (int path) { gRepPath = path; }

/* first i in [0, n) with rid[i] >= r, n if there is none: rid[] ascends, the scan's output being in (read, pos) order */
__device__ __forceinline__ U64 mgRepLowerBound (const U32 *__restrict__ rid, U64 n, U32 r)
{
  U64 lo = 0, hi = n;
  while (lo < hi) { const U64 mid = lo + (hi - lo) / 2; if (rid[mid] < r) lo = mid + 1; else hi = mid; }
  return lo;
}

/* flag[i] = modimizer i was found, for i < n; flag[n] = 0: the scan over n + 1 flags leaves the total in place[n] */
__global__ void mgRepFlagKernel (const U32 *__restrict__ ix, U64 n, U32 *__restrict__ flag)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= n ; i += (U64) gridDim.x * blockDim.x) flag[i] = i < n && ix[i] != 0; }

/* base[r] = found modimizers before read r's first one, r = 0 .. nReads (place[]: the exclusive scan of the flags, n + 1 entries) */
__global__ void mgRepReadBaseKernel (const U32 *__restrict__ rid, U64 n, U32 nReads, const U32 *__restrict__ place, U32 *__restrict__ base)
{ for (U64 r = (U64) blockIdx.x * blockDim.x + threadIdx.x ; r <= nReads ; r += (U64) gridDim.x * blockDim.x) base[r] = place[mgRepLowerBound (rid, n, (U32) r)]; }

__global__ void mgRepWidenKernel (const U32 *__restrict__ a, U64 n, U64 *__restrict__ out)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x) out[i] = a[i]; }

/* ---- -R ---- */

/* stat[0] += hits found, stat[1] = max (loc + 1); last[x] = max ((loc << 1) | isF); minNZ[x] = min (loc > 0) */
__global__ __launch_bounds__ (256)
void mgRepLocateKernel (const U32 *__restrict__ ix, const U32 *__restrict__ posF, U64 n, U32 *__restrict__ last, U32 *__restrict__ minNZ, U32 *__restrict__ stat)
{
  __shared__ U32 lds[4];
  U32 c = 0, top = 0;
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 x = ix[i];
      if (!x) continue;
      const U32 loc = posF[i] & MG_POS_MASK;
      atomicMax (&last[x], (loc << 1) | (posF[i] >> 31));
      if (loc) atomicMin (&minNZ[x], loc);
      ++c; if (loc + 1 > top) top = loc + 1;
    }
  c = mgBlockReduce<256, MgSum> (c, lds);
  if (!threadIdx.x && c) atomicAdd (&stat[0], c);
  top = mgBlockReduce<256, MgMax> (top, lds);
  if (!threadIdx.x && top) atomicMax (&stat[1], top);
}
/* stat[2] = the smallest loc of a hit that finds pos[index] non-zero (modrep.c:48): one above its entry's smallest non-zero loc */
__global__ void mgRepLocateDieKernel (const U32 *__restrict__ ix, const U32 *__restrict__ posF, U64 n, const U32 *__restrict__ minNZ, U32 *__restrict__ stat)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 x = ix[i], loc = posF[i] & MG_POS_MASK;
      if (x && loc > minNZ[x]) atomicMin (&stat[2], loc);
    }
}
__global__ void mgRepLocateUnpackKernel (const U32 *__restrict__ last, U64 m, int *__restrict__ pos, U8 *__restrict__ isF)
{ for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < m ; i += (U64) gridDim.x * blockDim.x) { pos[i] = (int) (last[i] >> 1); isF[i] = (U8) (last[i] & 1u); } }

/* ---- -s3: vote ---- */

/* modrep.c:197-202: the first MG_REP_VOTES found modimizers of a read vote */
__global__ void mgRepVoteKernel (const U32 *__restrict__ ix, const U32 *__restrict__ posF, const U32 *__restrict__ rid, U64 n, const U32 *__restrict__ place,
                                 const U32 *__restrict__ base, const U8 *__restrict__ refIsF, U32 *__restrict__ seqF, U32 *__restrict__ seqR)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 x = ix[i];
      if (!x) continue;
      const U32 r = rid[i];
      if (place[i] - base[r] >= MG_REP_VOTES) continue;
      const bool f = (posF[i] & MG_FWD_BIT) != 0;
      atomicAdd (f == (refIsF[x] != 0) ? &seqF[r] : &seqR[r], 1u);
    }
}
/* modrep.c:204,215: per read n, bad, flip; good[r] for r < nReads, good[nReads] = 0 */
__global__ void mgRepVerdictKernel (const U32 *__restrict__ base, const U32 *__restrict__ seqF, const U32 *__restrict__ seqR, U32 nReads,
                                    U32 *__restrict__ nOut, U32 *__restrict__ bad, U32 *__restrict__ flip, U32 *__restrict__ good)
{
  for (U64 r = (U64) blockIdx.x * blockDim.x + threadIdx.x ; r <= nReads ; r += (U64) gridDim.x * blockDim.x)
    { if (r == nReads) { good[r] = 0; continue; }
      const U32 found = base[r + 1] - base[r], n = found < MG_REP_VOTES ? found : MG_REP_VOTES;
      const U32 f = seqF[r], v = seqR[r];
      const U32 b = n < MG_REP_VOTES || (f > MG_REP_MIXED && v > MG_REP_MIXED);
      nOut[r] = n; bad[r] = b; flip[r] = !b && f < v; good[r] = !b;
    }
}

/* ---- -s3: orient ---- */

/* good read g = goodPlace[r]: goodRead[g] = r, newLen[g] = its length; newLen[nGood] = 0 */
__global__ void mgRepCompactKernel (const U32 *__restrict__ good, const U32 *__restrict__ goodPlace, const U64 *__restrict__ off, U32 nReads, U32 nGood,
                                    U32 *__restrict__ goodRead, U32 *__restrict__ newLen)
{
  for (U64 r = (U64) blockIdx.x * blockDim.x + threadIdx.x ; r <= nReads ; r += (U64) gridDim.x * blockDim.x)
    { if (r == nReads) { newLen[nGood] = 0; continue; }
      if (!good[r]) continue;
      const U32 g = goodPlace[r];
      goodRead[g] = (U32) r; newLen[g] = (U32) (off[r + 1] - off[r]);
    }
}
__device__ __forceinline__ U32 mgRepBaseAt (const U32 *__restrict__ packed, U64 i) { return (packed[i >> 4] >> (30u - 2u * (U32) (i & 15))) & 3u; }
/* a lane per word of the oriented batch: its 16 bases from the good reads, base p of a flipped read being 3 - base (len - 1 - p) of its source
   (modrep.c:215-220); the words past the last base (the pad, mgPackedWords) are zero */
__global__ void mgRepOrientKernel (const U32 *__restrict__ packed, const U64 *__restrict__ off, const U32 *__restrict__ goodRead, const U32 *__restrict__ newOff,
                                   const U32 *__restrict__ flip, U32 nGood, U64 newTotal, U64 nWords, U32 *__restrict__ out)
{
  for (U64 j = (U64) blockIdx.x * blockDim.x + threadIdx.x ; j < nWords ; j += (U64) gridDim.x * blockDim.x)
    { U32 wv = 0;
      const U64 b0 = j * 16;
      if (b0 < newTotal)
        { U32 lo = 0, hi = nGood - 1;                                /* the last g with newOff[g] <= b0 */
          while (lo < hi) { const U32 mid = lo + (hi - lo + 1) / 2; if ((U64) newOff[mid] <= b0) lo = mid; else hi = mid - 1; }
          U32 g = lo;
          for (U32 t = 0 ; t < 16 && b0 + t < newTotal ; ++t)
            { const U64 b = b0 + t;
              while (g + 1 < nGood && b >= (U64) newOff[g + 1]) ++g;
              const U32 r = goodRead[g], len = newOff[g + 1] - newOff[g], p = (U32) (b - newOff[g]);
              const bool fl = flip[r] != 0;
              U32 v = mgRepBaseAt (packed, off[r] + (fl ? len - 1 - p : p));
              if (fl) v = 3u - v;
              wv |= v << (30u - 2u * t);
            }
        }
      out[j] = wv;
    }
}

/* ---- -s3: hits ---- */

/* modrep.c:227-232: the found modimizers of the oriented batch, in order, behind the at0 hits the run holds */
__global__ void mgRepHitKernel (const U32 *__restrict__ ix, const U32 *__restrict__ posF, const U32 *__restrict__ rid, U64 n, const U32 *__restrict__ place,
                                U64 at0, U32 goodBase, U32 *__restrict__ hitK, U32 *__restrict__ hitX, U32 *__restrict__ hitRead)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 x = ix[i];
      if (!x) continue;
      const U64 at = at0 + place[i];
      hitK[at] = x; hitX[at] = posF[i] & MG_POS_MASK; hitRead[at] = goodBase + rid[i];
    }
}

/* ---- -s3: after the file ---- */

/* sorted[0 .. n): hit ordinals by k, in hit order inside a k: ++n[k] per hit (modrep.c:228), ++nPre[k] when the hit before it in the
   order shares k and read (modrep.c:229: the second and later occurrence in one read) */
__global__ void mgRepTallyKernel (const U32 *__restrict__ sorted, U64 n, const U32 *__restrict__ hitK, const U32 *__restrict__ hitRead,
                                  U32 *__restrict__ modN, U32 *__restrict__ modNPre)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 a = sorted[i], k = hitK[a];
      atomicAdd (&modN[k], 1u);
      if (i) { const U32 q = sorted[i - 1]; if (hitK[q] == k && hitRead[q] == hitRead[a]) atomicAdd (&modNPre[k], 1u); }
    }
}
/* modrep.c:238-244 over i = 0 .. max - 1: counts[3] = nMod, nDup, tDup; n[i] = 0 where nPre[i] */
__global__ __launch_bounds__ (256)
void mgRepCountKernel (U32 *__restrict__ modN, const U32 *__restrict__ modNPre, U32 max, U32 *__restrict__ counts)
{
  __shared__ U32 lds[4];
  U32 c[3] = { 0, 0, 0 };
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < max ; i += (U64) gridDim.x * blockDim.x)
    { const U32 p = modNPre[i];
      if (p) { ++c[1]; c[2] += p; modN[i] = 0; } else ++c[0];
    }
  for (int j = 0 ; j < 3 ; ++j)
    { const U32 s = mgBlockReduce<256, MgSum> (c[j], lds);
      if (!threadIdx.x && s) atomicAdd (&counts[j], s);
    }
}
/* modrep.c:253-255: readMax[g] = the largest n[k] over good read g's hits */
__global__ void mgRepReadMaxKernel (const U32 *__restrict__ hitK, const U32 *__restrict__ hitRead, U64 n, const U32 *__restrict__ modN, U32 *__restrict__ readMax)
{
  for (U64 h = (U64) blockIdx.x * blockDim.x + threadIdx.x ; h < n ; h += (U64) gridDim.x * blockDim.x)
    { const U32 v = modN[hitK[h]]; if (v) atomicMax (&readMax[hitRead[h]], v); }
}
/* modrep.c:256: a read whose maximum is 0 starts the fold again: fold[0] = 1 + the last such read, fold[1] = the minimum after it */
__global__ void mgRepLastZeroKernel (const U32 *__restrict__ readMax, U32 nGood, U32 *__restrict__ fold)
{ for (U64 g = (U64) blockIdx.x * blockDim.x + threadIdx.x ; g < nGood ; g += (U64) gridDim.x * blockDim.x) if (!readMax[g]) atomicMax (&fold[0], (U32) g + 1); }
__global__ void mgRepMinAfterKernel (const U32 *__restrict__ readMax, U32 nGood, U32 *__restrict__ fold)
{ const U32 from = fold[0]; for (U64 g = from + (U64) blockIdx.x * blockDim.x + threadIdx.x ; g < nGood ; g += (U64) gridDim.x * blockDim.x) atomicMin (&fold[1], readMax[g]); }

/* ---------------------------------------------------------------------------------------- */

/* the modimizers of a device batch scanned with scanWith (0: the set's own hasher), in (read, pos) order, and their indices in ms (0: absent):
   the library's seed list (mgSeedsOfBatch) from modrep's own first guess, its arrays handed to the scratch */
MgStatus mgRepSeedList (MgDevScratch &scratch, Modset *ms, const Seqhash *scanWith, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, MgRepSeeds *o, hipStream_t st)
{
  const int w = (scanWith ? scanWith : ms->hasher)->w;
  U64 guess = total / (U64) (w > 0 ? w : 1) * 2 + 4096; if (guess > total + 16) guess = total + 16;
  *o = MgRepSeeds ();
  const MgStatus s = mgSeedsOfBatch (ms, scanWith, 0, dPacked, total, dOff, nReads, guess, o, &o->n, (void *) st);
  scratch.adopt (o->ix); scratch.adopt (o->posF); scratch.adopt (o->rid);
  if (s) return s;
  if (o->n >= 0xfffffff0ull) { mgSetError ("modrep: %llu modimizers in one batch (at most 2^32 - 17)", (unsigned long long) o->n); return MG_ERR_ARG; }
  return MG_OK;
}

/* host bases -> packed words and offsets in the scratch */
MgStatus mgRepUpload (MgDevScratch &scratch, const char *bases, const int64_t *offsets, U32 nReads, U64 total, U32 **dPacked, U64 **dOff, hipStream_t st)
{
  MgStatus s;
  if (scratch.get (dPacked, mgPackedWords (total)) || scratch.get (dOff, (size_t) nReads + 1)) return MG_ERR_HIP;
  if ((s = mgUploadPack (bases, total, *dPacked, (void *) st))) return s;
  if (hipMemcpyAsync (*dOff, offsets, ((size_t) nReads + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess) return scratch.fail ();
  return MG_OK;
}

/* ---- -R ---- */

extern "C" void mgRepRefDestroy (MgRepRef *ref)
{
  if (!ref) return;
  if (ref->ownsMs && ref->ms) { Seqhash *sh = ref->ms->hasher; modsetDestroy (ref->ms); if (sh) mgSeqhashDestroy (sh); }
  free (ref->pos); free (ref->isF); free (ref);
}

extern "C" MgRepRef *mgRepRefFromArrays (Modset *ms, const char *bases, int64_t len, FILE *err)
{
  static_assert (sizeof (bool) == 1, "isF[] is downloaded as bytes");
  if (!ms || !ms->hasher || len < 0 || (len && !bases) || len >= (int64_t) 0x7ffffff0) { mgSetError ("mgRepRefFromArrays: invalid arguments"); return 0; }
  if (mgEnsureDevice ()) return 0;
  hipStream_t st = 0;
  const size_t m = (size_t) ms->max + 1;
  const int64_t offsets[2] = { 0, len };
  MgDevScratch scratch ("modrep -R on the device");
  U32 *dPacked, *dLast, *dMinNZ, *dStat; U64 *dOff; int *dPos; U8 *dIsF;
  MgRepSeeds a;
  if (mgRepUpload (scratch, bases, offsets, 1, (U64) len, &dPacked, &dOff, st) || mgRepSeedList (scratch, ms, 0, dPacked, (U64) len, dOff, 1, &a, st)) return 0;
  if (scratch.get (&dLast, m) || scratch.get (&dMinNZ, m) || scratch.get (&dStat, 4) || scratch.get (&dPos, m) || scratch.get (&dIsF, m)) return 0;
  const U32 stat0[4] = { 0, 0, 0xffffffffu, 0 };
  if (hipMemsetAsync (dLast, 0, m * 4, st) != hipSuccess || hipMemsetAsync (dMinNZ, 0xff, m * 4, st) != hipSuccess
      || hipMemcpyAsync (dStat, stat0, 16, hipMemcpyHostToDevice, st) != hipSuccess) { scratch.fail (); return 0; }
  if (a.n)
    { hipLaunchKernelGGL (mgRepLocateKernel, dim3 (mgGrid (a.n)), dim3 (256), 0, st, a.ix, a.posF, a.n, dLast, dMinNZ, dStat);
      hipLaunchKernelGGL (mgRepLocateDieKernel, dim3 (mgGrid (a.n)), dim3 (256), 0, st, a.ix, a.posF, a.n, dMinNZ, dStat);
    }
  hipLaunchKernelGGL (mgRepLocateUnpackKernel, dim3 (mgGrid (m)), dim3 (256), 0, st, dLast, (U64) m, dPos, dIsF);
  U32 stat[4];
  if (hipGetLastError () != hipSuccess || hipMemcpyAsync (stat, dStat, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess) { scratch.fail (); return 0; }
  if (stat[2] != 0xffffffffu) { mgSetError ("duplicate mod entry at position %d in ref", (int) stat[2]); return 0; }      /* modrep.c:48 */
  MgRepRef *ref = (MgRepRef *) calloc (1, sizeof (MgRepRef));
  if (ref) { ref->pos = (int *) malloc (m * sizeof (int)); ref->isF = (bool *) malloc (m); }
  if (!ref || !ref->pos || !ref->isF) { mgRepRefDestroy (ref); mgSetError ("mgRepRefFromArrays: out of memory"); return 0; }
  if (hipMemcpy (ref->pos, dPos, m * sizeof (int), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (ref->isF, dIsF, m, hipMemcpyDeviceToHost) != hipSuccess)
    { mgRepRefDestroy (ref); scratch.fail (); return 0; }
  ref->ms = ms; ref->len = (int) stat[1];
  if (err) fprintf (err, "found %d of %d locations in ref length %llu\n", (int) stat[0], (int) ms->max, (unsigned long long) len);      /* modrep.c:58-59 */
  return ref;
}

/* a .mod file, gzip or plain: 0 with the program's message if it cannot be opened */
Modset *mgRepReadSet (const char *modFile)
{
  FILE *f = mgFzOpen (modFile, "r");
  if (!f) { mgSetError ("failed to open mod file %s", modFile); return 0; }      /* modrep.c:34,180 */
  Modset *ms = modsetRead (f);
  fclose (f);
  return ms;
}
void mgRepSetDestroy (Modset *ms) { if (ms) { Seqhash *sh = ms->hasher; modsetDestroy (ms); if (sh) mgSeqhashDestroy (sh); } }

extern "C" MgRepRef *mgRepRefCreate (const char *seqFile, const char *modFile, FILE *err)
{
  if (!seqFile || !modFile) { mgSetError ("mgRepRefCreate: invalid arguments"); return 0; }
  Modset *ms = mgRepReadSet (modFile);
  if (!ms) { if (!mgLastError ()[0]) mgSetError ("failed to read reference modset from file %s", modFile); return 0; }      /* modrep.c:36 */
  MgSeqReader *r = mgSeqOpen (seqFile);
  if (!r) { mgSetError ("can't open reference sequence file %s", seqFile); mgRepSetDestroy (ms); return 0; }      /* modrep.c:42 */
  MgSeqBatch b, b2;
  MgRepRef *ref = 0;
  if (mgSeqNextBatch (r, 1, &b) <= 0) mgSetError ("can't read reference sequence");      /* modrep.c:55 */
  else
    { bool more = b.nSeq > 1;
      if (!more && mgSeqNextBatch (r, 1, &b2) > 0) { more = true; mgSeqBatchFree (&b2); }
      ref = mgRepRefFromArrays (ms, b.bases + b.offsets[0], b.offsets[1] - b.offsets[0], more ? 0 : err);      /* (the duplicate check comes first: modrep.c:48,56) */
      if (ref && more) { mgRepRefDestroy (ref); ref = 0; mgSetError ("multiple sequences in ref file - only one allowed"); }      /* modrep.c:56 */
      mgSeqBatchFree (&b);
    }
  mgSeqClose (r);
  if (!ref) { mgRepSetDestroy (ms); return 0; }
  ref->ownsMs = 1;
  return ref;
}

/* ---- -s3 ---- */

extern "C" MgRepRun *mgRepRunBegin (MgRepRef *ref, Modset *ms)
{
  gRepPath = -1;
  if (!ref || !ref->ms || !ref->ms->hasher || !ref->isF || !ms || !ms->hasher) { mgSetError ("mgRepRunBegin: invalid arguments"); return 0; }
  if (ref->ms->hasher->k != ms->hasher->k)
    { mgSetError ("mgRepRunBegin: the reference set has k %d, the second set k %d (the reads are scanned with the reference set's hasher)", ref->ms->hasher->k, ms->hasher->k); return 0; }
  if (mgEnsureDevice ()) return 0;
  MgRepRun *run = new MgRepRun ();
  run->ref = ref; run->ms = ms;
  const size_t m = (size_t) ref->ms->max + 1;
  if (hipGetDevice (&run->device) != hipSuccess || run->refIsF.reserve (m, m, "modrep -s3: the reference's strands")
      || hipMemcpy (run->refIsF.p, ref->isF, m, hipMemcpyHostToDevice) != hipSuccess)
    { if (!mgLastError ()[0]) mgHipFail (hipGetLastError (), "mgRepRunBegin"); delete run; return 0; }
  run->hitStart.push_back (0);
  return run;
}

/* the run's three hit arrays with room for `want` hits, the nHit held so far kept */
static MgStatus mgRepGrowHits (MgRepRun *run, U64 want)
{
  if (run->hitK.cap >= want) return MG_OK;
  const size_t cap = (size_t) (want + (run->nHit ? want / 2 : 0) + 1024);      /* (a file that is one batch gets what it needs; one of many batches grows by halves) */
  MgDevBuf<U32> *bufs[3] = { &run->hitK, &run->hitX, &run->hitRead };
  for (int j = 0 ; j < 3 ; ++j)
    { MgDevBuf<U32> nb; MgStatus s;
      if ((s = nb.reserve (cap, cap, "modrep -s3: the file's hits"))) return s;
      if (run->nHit && hipMemcpy (nb.p, bufs[j]->p, run->nHit * 4, hipMemcpyDeviceToDevice) != hipSuccess) { nb.drop (); return mgHipFail (hipGetLastError (), "modrep -s3: the file's hits"); }
      bufs[j]->drop (); *bufs[j] = nb;
    }
  return MG_OK;
}

static int mgRepRunAddOnDevice (MgRepRun *run, const char *bases, const int64_t *offsets, U32 nReads, FILE *out)
{
  hipStream_t st = 0;
  const U64 total = (U64) offsets[nReads];
  MgDevScratch scratch ("modrep -s3 on the device");
  U32 *dPacked, *flag, *place, *base, *dF, *dR, *dN, *dBad, *dFlip, *good, *goodPlace; U64 *dOff;
  MgRepSeeds a;
  if (mgRepUpload (scratch, bases, offsets, nReads, total, &dPacked, &dOff, st) || mgRepSeedList (scratch, run->ref->ms, 0, dPacked, total, dOff, nReads, &a, st)) return -1;
  const size_t nr = nReads;
  if (scratch.get (&flag, a.n + 1) || scratch.get (&place, a.n + 1) || scratch.get (&base, nr + 1) || scratch.get (&dF, nr) || scratch.get (&dR, nr) || scratch.get (&dN, nr)
      || scratch.get (&dBad, nr) || scratch.get (&dFlip, nr) || scratch.get (&good, nr + 1) || scratch.get (&goodPlace, nr + 1)) return -1;
  if (hipMemsetAsync (dF, 0, nr * 4, st) != hipSuccess || hipMemsetAsync (dR, 0, nr * 4, st) != hipSuccess) { scratch.fail (); return -1; }
  hipLaunchKernelGGL (mgRepFlagKernel, dim3 (mgGrid (a.n + 1)), dim3 (256), 0, st, a.ix, a.n, flag);
  if (mgExclusiveScan (scratch, flag, place, a.n + 1, st)) return -1;
  hipLaunchKernelGGL (mgRepReadBaseKernel, dim3 (mgGrid (nr + 1)), dim3 (256), 0, st, a.rid, a.n, nReads, place, base);
  if (a.n) hipLaunchKernelGGL (mgRepVoteKernel, dim3 (mgGrid (a.n)), dim3 (256), 0, st, a.ix, a.posF, a.rid, a.n, place, base, run->refIsF.p, dF, dR);
  hipLaunchKernelGGL (mgRepVerdictKernel, dim3 (mgGrid (nr + 1)), dim3 (256), 0, st, base, dF, dR, nReads, dN, dBad, dFlip, good);
  U32 nGood = 0;
  if (hipGetLastError () != hipSuccess) { scratch.fail (); return -1; }
  if (mgExclusiveScan (scratch, good, goodPlace, nr + 1, st, &nGood)) return -1;
  std::vector<U32> hN (nr), hF (nr), hR (nr), hBad (nr), hFlip (nr);
  if (hipMemcpy (hN.data (), dN, nr * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (hF.data (), dF, nr * 4, hipMemcpyDeviceToHost) != hipSuccess
      || hipMemcpy (hR.data (), dR, nr * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (hBad.data (), dBad, nr * 4, hipMemcpyDeviceToHost) != hipSuccess
      || hipMemcpy (hFlip.data (), dFlip, nr * 4, hipMemcpyDeviceToHost) != hipSuccess) { scratch.fail (); return -1; }
  const int read0 = (int) run->n.size ();
  const U32 good0 = (U32) run->goodI.size ();
  U32 hostGood = 0;
  for (U32 r = 0 ; r < nReads ; ++r)
    { run->n.push_back ((int) hN[r]); run->seqF.push_back ((int) hF[r]); run->seqR.push_back ((int) hR[r]);
      run->bad.push_back ((U8) hBad[r]); run->isF.push_back ((U8) (!hBad[r] && !hFlip[r]));
      const int len = (int) (offsets[r + 1] - offsets[r]);
      if (hBad[r])
        { ++run->nBad;
          if (out) fprintf (out, "BADREAD %5d len %5d n %d F %4d R %4d\n", read0 + (int) r + 1, len, (int) hN[r], (int) hF[r], (int) hR[r]);      /* modrep.c:206-207 */
        }
      else { run->goodI.push_back (read0 + (int) r); run->goodLen.push_back (len); ++hostGood; }
    }
  if (hostGood != nGood) { mgSetError ("modrep -s3: the device counted %u good reads, their flags say %u", nGood, hostGood); return -1; }
  if (!nGood) return 0;

  U32 *goodRead, *newLen, *newOff, *dPacked2, *flag2, *place2, *hs; U64 *newOff64;
  U32 newTotal = 0;
  const size_t ng = nGood;
  if (scratch.get (&goodRead, ng) || scratch.get (&newLen, ng + 1) || scratch.get (&newOff, ng + 1) || scratch.get (&newOff64, ng + 1) || scratch.get (&hs, ng + 1)) return -1;
  hipLaunchKernelGGL (mgRepCompactKernel, dim3 (mgGrid (nr + 1)), dim3 (256), 0, st, good, goodPlace, dOff, nReads, nGood, goodRead, newLen);
  if (mgExclusiveScan (scratch, newLen, newOff, ng + 1, st, &newTotal)) return -1;      /* (a batch holds fewer than 2^32 bases: mgRepRunAdd) */
  const U64 nWords = mgPackedWords (newTotal);
  if (scratch.get (&dPacked2, nWords)) return -1;
  hipLaunchKernelGGL (mgRepWidenKernel, dim3 (mgGrid (ng + 1)), dim3 (256), 0, st, newOff, (U64) ng + 1, newOff64);
  hipLaunchKernelGGL (mgRepOrientKernel, dim3 (mgGrid (nWords)), dim3 (256), 0, st, dPacked, dOff, goodRead, newOff, dFlip, nGood, (U64) newTotal, nWords, dPacked2);
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st) != hipSuccess) { scratch.fail (); return -1; }
  MgRepSeeds b;
  if (mgRepSeedList (scratch, run->ms, run->ref->ms->hasher, dPacked2, newTotal, newOff64, nGood, &b, st)) return -1;
  U32 nHitB = 0;
  if (scratch.get (&flag2, b.n + 1) || scratch.get (&place2, b.n + 1)) return -1;
  hipLaunchKernelGGL (mgRepFlagKernel, dim3 (mgGrid (b.n + 1)), dim3 (256), 0, st, b.ix, b.n, flag2);
  if (mgExclusiveScan (scratch, flag2, place2, b.n + 1, st, &nHitB)) return -1;
  if (run->nHit + nHitB >= 0xfffffff0ull) { mgSetError ("modrep -s3: more than 2^32 - 17 hits in one file"); return -1; }
  if (mgRepGrowHits (run, run->nHit + nHitB)) return -1;
  hipLaunchKernelGGL (mgRepReadBaseKernel, dim3 (mgGrid (ng + 1)), dim3 (256), 0, st, b.rid, b.n, nGood, place2, hs);
  if (nHitB) hipLaunchKernelGGL (mgRepHitKernel, dim3 (mgGrid (b.n)), dim3 (256), 0, st, b.ix, b.posF, b.rid, b.n, place2, run->nHit, good0, run->hitK.p, run->hitX.p, run->hitRead.p);
  std::vector<U32> hHs (ng + 1);
  if (hipGetLastError () != hipSuccess || hipMemcpy (hHs.data (), hs, (ng + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) { scratch.fail (); return -1; }
  for (U32 g = 1 ; g <= nGood ; ++g) run->hitStart.push_back (run->nHit + hHs[g]);
  run->nHit += nHitB;
  return 0;
}

extern "C" int mgRepRunAdd (MgRepRun *run, const char *bases, const int64_t *offsets, int nReads, FILE *out)
{
  gRepPath = -1;
  if (!run || nReads < 0 || (nReads && (!offsets || offsets[0] != 0 || (offsets[nReads] && !bases)))) { mgSetError ("mgRepRunAdd: invalid arguments"); return -1; }
  if (!nReads) return 0;
  if ((U64) offsets[nReads] >= 0xffffff00ull || run->n.size () + (size_t) nReads >= (size_t) INT_MAX)
    { mgSetError ("mgRepRunAdd: a batch holds fewer than 2^32 - 256 bases, a file fewer than 2^31 - 1 reads"); return -1; }
  for (int r = 0 ; r < nReads ; ++r)
    if (offsets[r + 1] < offsets[r] || offsets[r + 1] - offsets[r] > (int64_t) INT_MAX) { mgSetError ("mgRepRunAdd: bad read offsets"); return -1; }
  int cur = 0;
  if (mgEnsureDevice ()) return -1;
  if (hipGetDevice (&cur) != hipSuccess || cur != run->device) { mgSetError ("mgRepRunAdd: the run was begun on GPU %d, the calling thread is on GPU %d", run->device, cur); return -1; }
  return mgRepRunAddOnDevice (run, bases, offsets, (U32) nReads, out) ? mgFailedWith ("mgRepRunAdd failed") : 0;
}

extern "C" void mgRepResultFree (MgRepResult *res)
{
  if (!res) return;
  free (res->n); free (res->seqF); free (res->seqR); free (res->bad); free (res->isF); free (res->modN); free (res->modNPre);
  free (res->goodI); free (res->goodLen); free (res->hitStart); free (res->hitK); free (res->hitX);
  memset (res, 0, sizeof (*res));
}

static int mgRepFinishOnDevice (MgRepRun *run, FILE *err, MgRepResult *res)
{
  hipStream_t st = 0;
  const U32 max = run->ms->max, nGood = (U32) run->goodI.size ();
  const size_t m = (size_t) max + 1;
  const U64 N = run->nHit;
  MgDevScratch scratch ("modrep -s3: the end of the file");
  U32 *modN, *modNPre, *counts, *readMax, *fold, *sorted = 0;
  if (scratch.get (&modN, m) || scratch.get (&modNPre, m) || scratch.get (&counts, 4) || scratch.get (&readMax, (size_t) nGood + 1) || scratch.get (&fold, 2)) return -1;
  const U32 fold0[2] = { 0, 0xffffffffu };
  if (hipMemsetAsync (modN, 0, m * 4, st) != hipSuccess || hipMemsetAsync (modNPre, 0, m * 4, st) != hipSuccess || hipMemsetAsync (counts, 0, 16, st) != hipSuccess
      || hipMemsetAsync (readMax, 0, ((size_t) nGood + 1) * 4, st) != hipSuccess || hipMemcpyAsync (fold, fold0, 8, hipMemcpyHostToDevice, st) != hipSuccess) { scratch.fail (); return -1; }
  if (N)
    { if (mgRefStableSort (scratch, run->hitK.p, 0, (U32) N, mgKeyBits (max), &sorted, st)) return -1;
      hipLaunchKernelGGL (mgRepTallyKernel, dim3 (mgGrid (N)), dim3 (256), 0, st, sorted, N, run->hitK.p, run->hitRead.p, modN, modNPre);
    }
  if (max) hipLaunchKernelGGL (mgRepCountKernel, dim3 (mgGrid (max, 256, 1024)), dim3 (256), 0, st, modN, modNPre, max, counts);
  if (N) hipLaunchKernelGGL (mgRepReadMaxKernel, dim3 (mgGrid (N)), dim3 (256), 0, st, run->hitK.p, run->hitRead.p, N, modN, readMax);
  if (nGood)
    { hipLaunchKernelGGL (mgRepLastZeroKernel, dim3 (mgGrid (nGood)), dim3 (256), 0, st, readMax, nGood, fold);
      hipLaunchKernelGGL (mgRepMinAfterKernel, dim3 (mgGrid (nGood)), dim3 (256), 0, st, readMax, nGood, fold);
    }
  U32 hCounts[4], hFold[2];
  if (hipGetLastError () != hipSuccess || hipMemcpyAsync (hCounts, counts, 16, hipMemcpyDeviceToHost, st) != hipSuccess
      || hipMemcpyAsync (hFold, fold, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess) { scratch.fail (); return -1; }
  const int nRead = (int) run->n.size (), nMod = (int) hCounts[0], nDup = (int) hCounts[1], tDup = (int) hCounts[2];
  const int minMax = (!nGood || hFold[0] == nGood) ? 0 : (int) hFold[1];      /* the last good read's maximum is 0, or there is none: 0 */
  if (err)
    { fprintf (err, "read %d reads, %d bad, %d good: ", nRead, run->nBad, (int) nGood);                                          /* modrep.c:236 */
      fprintf (err, "mods total %d good %d dup %d avdup %.1f\n", (int) max, nMod, nDup, nDup ? (tDup / (double) nDup) : 0.);   /* modrep.c:245-246 */
      fprintf (err, "minimum max for a read is %d\n", minMax);                                                                  /* modrep.c:258 */
    }
  if (!res) return 0;
  memset (res, 0, sizeof (*res));
  res->nRead = nRead; res->nBad = run->nBad; res->nGood = (int) nGood; res->max = max;
  res->nMod = nMod; res->nDup = nDup; res->tDup = tDup; res->minMax = minMax;
  res->n = mgRepCopyOut<int> (run->n); res->seqF = mgRepCopyOut<int> (run->seqF); res->seqR = mgRepCopyOut<int> (run->seqR);
  res->bad = mgRepCopyOut<bool> (run->bad); res->isF = mgRepCopyOut<bool> (run->isF);
  res->goodI = mgRepCopyOut<int> (run->goodI); res->goodLen = mgRepCopyOut<int> (run->goodLen); res->hitStart = mgRepCopyOut<U64> (run->hitStart);
  res->modN = (int *) malloc (m * sizeof (int)); res->modNPre = (int *) malloc (m * sizeof (int));
  res->hitK = (int *) malloc ((N + 1) * sizeof (int)); res->hitX = (int *) malloc ((N + 1) * sizeof (int));
  if (!res->n || !res->seqF || !res->seqR || !res->bad || !res->isF || !res->goodI || !res->goodLen || !res->hitStart || !res->modN || !res->modNPre || !res->hitK || !res->hitX)
    { mgRepResultFree (res); mgSetError ("mgRepRunFinish: out of memory"); return -1; }
  if (hipMemcpy (res->modN, modN, m * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (res->modNPre, modNPre, m * 4, hipMemcpyDeviceToHost) != hipSuccess
      || (N && (hipMemcpy (res->hitK, run->hitK.p, N * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (res->hitX, run->hitX.p, N * 4, hipMemcpyDeviceToHost) != hipSuccess)))
    { mgRepResultFree (res); scratch.fail (); return -1; }
  return 0;
}

extern "C" int mgRepRunFinish (MgRepRun *run, FILE *err, MgRepResult *res)
{
  gRepPath = -1;
  if (!run) { mgSetError ("mgRepRunFinish: invalid arguments"); return -1; }
  int rc = -1, cur = 0;
  if (mgEnsureDevice ()) rc = -1;
  else if (hipGetDevice (&cur) != hipSuccess || cur != run->device) mgSetError ("mgRepRunFinish: the run was begun on GPU %d, the calling thread is on GPU %d", run->device, cur);
  else rc = mgRepFinishOnDevice (run, err, res);
  delete run;
  if (rc) return mgFailedWith ("mgRepRunFinish failed");
  gRepPath = 0;
  return 0;
}

extern "C" int mgRepAnalyze3File (MgRepRef *ref, const char *seqFile, const char *modFile, FILE *out, FILE *err, MgRepResult *res)
{
  gRepPath = -1;
  if (!ref || !seqFile || !modFile) { mgSetError ("mgRepAnalyze3File: invalid arguments"); return -1; }
  Modset *ms = mgRepReadSet (modFile);
  if (!ms) { if (!mgLastError ()[0]) mgSetError ("failed to read modset from file %s", modFile); return -1; }      /* modrep.c:182 */
  MgSeqReader *r = mgSeqOpen (seqFile);
  if (!r) { mgSetError ("can't open sequence file %s", seqFile); mgRepSetDestroy (ms); return -1; }      /* modrep.c:189 */
  MgRepRun *run = mgRepRunBegin (ref, ms);
  int rc = run ? 0 : -1;
  MgSeqBatch b;
  while (!rc && mgSeqNextBatch (r, MG_REP_FILE_BATCH, &b) > 0)
    { rc = mgRepRunAdd (run, b.bases, b.offsets, b.nSeq, out);
      mgSeqBatchFree (&b);
    }
  mgSeqClose (r);
  if (run) { const int rf = mgRepRunFinish (run, rc ? 0 : err, rc ? 0 : res); if (!rc) rc = rf; }
  mgRepSetDestroy (ms);
  if (rc) gRepPath = -1;
  return rc ? -1 : 0;
}
