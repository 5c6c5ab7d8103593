/* mg_report.hip — modutils' two reports on a set that is already built, and its text dump, on the device:
 *
 *   -d  reportDepths (modutils.c:65-77): per entry i of the set "MH\t%llx\t%d\t%u" (value, copy, depth), then the entry's depth in
 *       each of N other sets ("\t%u", 0 if absent), "\n";
 *   -P  refpaint (modutils.c:260-273): per record "painting %s length %d\n", then "  %d\t%d\n" (pos, depth) for every modimizer of the
 *       record that is in the set, in modRCnext order.
 * and, with the same formatter, the text form of the set itself:
 *   -wt (modutils.c:191-199): per entry i "%d\t%s\t%d\t%d\n" (i, the k letters of value[i], depth, info) behind the host's header line.
 *
 * The lookups are the library's batch finds (mgQueryReadsDevice: scan + find with positions; modsetFindBatchDevice), the depths are
 * gathered from the folded view of each set (host depth plus pending device counts, saturated: mgHookDeviceView), and the text itself
 * is made here, by one formatter that serves both reports.  It takes a chunk of at most MG_TEXT_CHUNK lines in three passes: every
 * line's length (one workgroup sums 1024 of them), an exclusive scan of the workgroup sums, and the bytes, each line written by one
 * lane at its offset.  A chunk's text is copied into page-locked blocks and written, in order, by a writer thread (mg_textout.c) while
 * the device goes on with the next chunk, so the memory a report takes does not grow with the set.
 *
 * Integer to text: digit counts by comparisons, decimal digits by a multiply-high with the reciprocal of 10 (exact for every 32-bit
 * value), hex digits from nibbles with the count from clz (%llx: lowercase, no leading zeros, 0 prints "0").
 */
#include <string.h>
#include <vector>
#include "mg_prefix.h"
#include "mg_internal.h"

#define MG_TEXT_THREADS 256
#define MG_TEXT_PER     4                                         /* lines per lane and pass */
#define MG_TEXT_BLOCK   (MG_TEXT_THREADS * MG_TEXT_PER)           /* lines per workgroup */
#define MG_TEXT_CHUNK   ((U64) 1 << 24)                           /* lines per chunk: bounds the text buffer (-d with one other set: ~0.5 GB) */
#define MG_HDR_BIT 0x80000000u                                    /* paint item: the header of read (item & ~MG_HDR_BIT), else a seed ordinal */

extern "C" void mgSetErrorText (const char *msg) { mgSetError ("%s", msg); }

/* ---------------------------------------------------------------------------------------- */
/* integer -> text                                                                            */

__device__ __forceinline__ U32 mgDecLen (U32 x)
{
  return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u)
         + (x >= 100000000u) + (x >= 1000000000u);
}
/* the n = mgDecLen (x) digits of x at p; returns p + n.  x / 10 = (x * 0xCCCCCCCD) >> 35 for every 32-bit x */
__device__ __forceinline__ char *mgPutDec (char *p, U32 x, U32 n)
{
  char *q = p + n;
  do { const U32 d = __umulhi (x, 0xCCCCCCCDu) >> 3; *--q = (char) ('0' + (x - d * 10u)); x = d; } while (q > p);
  return p + n;
}
__device__ __forceinline__ U32 mgHexLen (U64 v) { return v ? (67u - (U32) __clzll ((long long) v)) >> 2 : 1u; }
__device__ __forceinline__ char *mgPutHex (char *p, U64 v, U32 n)
{
  for (int i = (int) n - 1 ; i >= 0 ; --i)
    { const U32 nib = (U32) (v >> (4 * i)) & 15u; *p++ = (char) (nib < 10u ? '0' + nib : 'a' - 10 + nib); }
  return p;
}
__device__ __forceinline__ char *mgPutStr (char *p, const char *s, U32 n) { for (U32 i = 0 ; i < n ; ++i) p[i] = s[i]; return p + n; }

/* ---------------------------------------------------------------------------------------- */
/* the lines of the two reports                                                               */

/* -P: the batch's records and seeds in one order, item[j] (mgPaintItemsKernel) */
struct MgPaintLines {
  const U32 *item, *seedIx, *seedPosF;
  const U16 *depth1;                 /* the set's folded depths, entry i at [i - 1] */
  const U64 *readOff;                /* [nReads + 1], in bases */
  const char *ids; const U64 *idOff; /* id of read r: ids + idOff[r], 0-terminated */
  __device__ U32 idLen (U32 r) const { const char *s = ids + idOff[r]; U32 n = 0; while (s[n]) ++n; return n; }
  __device__ U32 len (U64 j) const
  {
    const U32 it = item[j];
    if (it & MG_HDR_BIT)
      { const U32 r = it & ~MG_HDR_BIT;
        return 9u + idLen (r) + 8u + mgDecLen ((U32) (readOff[r + 1] - readOff[r])) + 1u;         /* "painting %s length %d\n" */
      }
    const U32 ix = seedIx[it];
    if (!ix) return 0;                                                                             /* not in the set: no line */
    return 2u + mgDecLen (seedPosF[it] & MG_POS_MASK) + 1u + mgDecLen (depth1[ix - 1]) + 1u;      /* "  %d\t%d\n" */
  }
  __device__ void put (U64 j, char *p) const
  {
    const U32 it = item[j];
    if (it & MG_HDR_BIT)
      { const U32 r = it & ~MG_HDR_BIT;
        const U32 L = (U32) (readOff[r + 1] - readOff[r]);
        p = mgPutStr (p, "painting ", 9);
        p = mgPutStr (p, ids + idOff[r], idLen (r));
        p = mgPutStr (p, " length ", 8);
        p = mgPutDec (p, L, mgDecLen (L));
        *p = '\n';
        return;
      }
    const U32 ix = seedIx[it], pos = seedPosF[it] & MG_POS_MASK, d = depth1[ix - 1];
    *p++ = ' '; *p++ = ' ';
    p = mgPutDec (p, pos, mgDecLen (pos));
    *p++ = '\t';
    p = mgPutDec (p, d, mgDecLen (d));
    *p = '\n';
  }
};

/* -d: entry j of the chunk; oth[o * m + j] is its depth in other set o */
struct MgDepthLines {
  const U64 *value; const U16 *depth; const U8 *info; const U16 *oth; int nOth; U64 m;
  __device__ U32 len (U64 j) const
  {
    U32 n = 3u + mgHexLen (value[j]) + 3u + mgDecLen (depth[j]) + 1u;                             /* "MH\t%llx\t%d\t%u" ... "\n" */
    for (int o = 0 ; o < nOth ; ++o) n += 1u + mgDecLen (oth[(U64) o * m + j]);
    return n;
  }
  __device__ void put (U64 j, char *p) const
  {
    const U64 v = value[j]; const U32 d = depth[j];
    *p++ = 'M'; *p++ = 'H'; *p++ = '\t';
    p = mgPutHex (p, v, mgHexLen (v));
    *p++ = '\t'; *p++ = (char) ('0' + (info[j] & 3)); *p++ = '\t';                                /* msCopy = info & 3 */
    p = mgPutDec (p, d, mgDecLen (d));
    for (int o = 0 ; o < nOth ; ++o)
      { const U32 e = oth[(U64) o * m + j]; *p++ = '\t'; p = mgPutDec (p, e, mgDecLen (e)); }
    *p = '\n';
  }
};

/* -wt (modutils.c:196-198): entry j + 1 of the set, "%d\t%s\t%d\t%d\n" = index, the k letters of the value (seqhash.c:198-206: the low 2k
   bits, first base in the high ones), depth, info */
struct MgSetLines {
  const U64 *value; const U16 *depth; const U8 *info; int k;
  __device__ U32 len (U64 j) const { return mgDecLen ((U32) j + 1u) + 1u + (U32) k + 1u + mgDecLen (depth[j]) + 1u + mgDecLen (info[j]) + 1u; }
  __device__ void put (U64 j, char *p) const
  {
    const U64 v = value[j]; const U32 i = (U32) j + 1u, d = depth[j], f = info[j];
    p = mgPutDec (p, i, mgDecLen (i));
    *p++ = '\t';
    for (int b = k - 1 ; b >= 0 ; --b) *p++ = "acgt"[(v >> (2 * b)) & 3u];
    *p++ = '\t';
    p = mgPutDec (p, d, mgDecLen (d));
    *p++ = '\t';
    p = mgPutDec (p, f, mgDecLen (f));
    *p = '\n';
  }
};

/* ---------------------------------------------------------------------------------------- */
/* the formatter: length, scan, write                                                         */

/* pass 1: bytes of the workgroup's 1024 lines (j0 + b * 1024 ...) -> blockSum[b] */
template <class L>
__global__ __launch_bounds__ (MG_TEXT_THREADS) void mgTextLenKernel (L lines, U64 j0, U64 m, U32 *__restrict__ blockSum)
{
  __shared__ U32 lds[MG_TEXT_THREADS / 64];
  const U64 base = (U64) blockIdx.x * MG_TEXT_BLOCK;
  U32 s = 0;
  #pragma unroll
  for (int q = 0 ; q < MG_TEXT_PER ; ++q)
    { const U64 j = base + (U64) q * MG_TEXT_THREADS + threadIdx.x; if (j < m) s += lines.len (j0 + j); }
  s = mgBlockReduce<MG_TEXT_THREADS, MgSum> (s, lds);
  if (threadIdx.x == 0) blockSum[blockIdx.x] = s;
}

/* pass 2 (one workgroup, mgGroupSumKernel): blockOff[b] = exclusive sum of blockSum[0 .. b), blockOff[nb] = the chunk's bytes */

/* pass 3: the lines' bytes at their offsets (a line is written by one lane) */
template <class L>
__global__ __launch_bounds__ (MG_TEXT_THREADS) void mgTextWriteKernel (L lines, U64 j0, U64 m, const U64 *__restrict__ blockOff, char *__restrict__ out)
{
  __shared__ U32 lds[MG_TEXT_THREADS / 64];
  const U64 base = (U64) blockIdx.x * MG_TEXT_BLOCK;
  U64 at = blockOff[blockIdx.x];
  #pragma unroll 1
  for (int q = 0 ; q < MG_TEXT_PER ; ++q)
    { const U64 j = base + (U64) q * MG_TEXT_THREADS + threadIdx.x;
      const U32 n = j < m ? lines.len (j0 + j) : 0u;
      U32 tot;
      const U32 inc = mgBlockInclusive<MG_TEXT_THREADS, MgSum> (n, lds, &tot);
      if (n) lines.put (j0 + j, out + at + (inc - n));
      at += tot;
    }
}

/* ---------------------------------------------------------------------------------------- */
/* the small kernels of the two reports                                                       */

/* seedStart[r] = seeds of the reads before r (seeds come in read order); r in [0, nReads] */
__global__ void mgPaintStartKernel (const U32 *__restrict__ seedRead, U64 n, U32 nReads, U32 *__restrict__ seedStart)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= n ; i += (U64) gridDim.x * blockDim.x)
    { const U64 lo = i ? (U64) seedRead[i - 1] + 1 : 0, hi = i < n ? (U64) seedRead[i] : (U64) nReads;
      for (U64 r = lo ; r <= hi ; ++r) seedStart[r] = (U32) i;
    }
}
/* the output order: read r's header at seedStart[r] + r, seed i right after the headers of the reads up to its own */
__global__ void mgPaintItemsKernel (const U32 *__restrict__ seedRead, U64 n, U32 nReads, const U32 *__restrict__ seedStart, U32 *__restrict__ item)
{
  for (U64 t = (U64) blockIdx.x * blockDim.x + threadIdx.x ; t < n + nReads ; t += (U64) gridDim.x * blockDim.x)
    { if (t < n) item[t + seedRead[t] + 1] = (U32) t;
      else { const U32 r = (U32) (t - n); item[(U64) seedStart[r] + r] = MG_HDR_BIT | r; }
    }
}
/* a value wider than the other set's 2k bits is in no set of that k (every stored value is below 4^k) and must not reach its table:
   its hash would be another key, its bucket possibly past the table's end.  Such values are looked up as 0 and answered 0 below. */
__global__ void mgDepthGuardKernel (const U64 *__restrict__ value, U64 m, int kbits, U64 *__restrict__ key)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < m ; i += (U64) gridDim.x * blockDim.x)
    { const U64 v = value[i]; key[i] = (v >> kbits) ? 0ull : v; }
}
__global__ void mgDepthGatherKernel (const U64 *__restrict__ value, U64 m, int kbits, const U32 *__restrict__ idx, const U16 *__restrict__ depth1,
                                     U16 *__restrict__ out)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < m ; i += (U64) gridDim.x * blockDim.x)
    { const U32 ix = idx[i]; out[i] = ((value[i] >> kbits) || !ix) ? (U16) 0 : depth1[ix - 1]; }
}

/* ---------------------------------------------------------------------------------------- */
/* host side                                                                                  */

/* device scratch of a report call, grow-only */
struct MgReportBufs {
  U32 *blockSum = 0; U64 *blockOff = 0; U64 *hTotal = 0;
  MgDevBuf<char> text, ids;
  MgSeedBufs seeds = { 0, 0, 0, 0, 0 };                   /* the batch's seed list (mgSeedsOfBatch) */
  MgDevBuf<U32> start, item;
  MgDevBuf<U64> idOff;
  ~MgReportBufs ()
  { (void) hipFree (blockSum); (void) hipFree (blockOff); (void) hipHostFree (hTotal);
    text.drop (); ids.drop (); mgSeedBufsFree (&seeds); start.drop (); item.drop (); idOff.drop ();
  }
};
static inline size_t mgRoomFor (size_t want) { return want + want / 8 + 64; }      /* what a report's buffers grow to */
static MgStatus mgReportBufsInit (MgReportBufs *b)
{
  if (b->blockSum) return MG_OK;
  const U64 nb = MG_TEXT_CHUNK / MG_TEXT_BLOCK + 1;
  MG_HIP (hipMalloc ((void **) &b->blockSum, nb * sizeof (U32)));
  MG_HIP (hipMalloc ((void **) &b->blockOff, (nb + 1) * sizeof (U64)));
  MG_HIP (hipHostMalloc ((void **) &b->hTotal, 64, hipHostMallocDefault));
  return MG_OK;
}

/* n lines through the formatter, MG_TEXT_CHUNK at a time, each chunk's text to the writer */
template <class L>
static MgStatus mgTextFormat (const L &lines, U64 n, MgReportBufs *b, MgTextOut *w, hipStream_t st)
{
  MgStatus s = mgReportBufsInit (b); if (s) return s;
  for (U64 j0 = 0 ; j0 < n ; j0 += MG_TEXT_CHUNK)
    { const U64 m = n - j0 < MG_TEXT_CHUNK ? n - j0 : MG_TEXT_CHUNK;
      const U32 nb = (U32) ((m + MG_TEXT_BLOCK - 1) / MG_TEXT_BLOCK);
      MG_LAUNCH (MG_K_TEXT_LEN, st, mgTextLenKernel<L>, dim3 (nb), dim3 (MG_TEXT_THREADS), 0, st, lines, j0, m, b->blockSum);
      MG_LAUNCH (MG_K_TEXT_SCAN, st, (mgGroupSumKernel<U32, U64>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, b->blockSum, b->blockOff, nb, b->blockOff + nb);
      MG_HIP (hipMemcpyAsync (b->hTotal, b->blockOff + nb, 8, hipMemcpyDeviceToHost, st));
      MG_HIP (hipStreamSynchronize (st));
      const U64 bytes = *(volatile U64 *) b->hTotal;
      if (!bytes) continue;
      if ((s = b->text.reserve (bytes, mgRoomFor (bytes), "report text"))) return s;
      MG_LAUNCH (MG_K_TEXT_WRITE, st, mgTextWriteKernel<L>, dim3 (nb), dim3 (MG_TEXT_THREADS), 0, st, lines, j0, m, b->blockOff, b->text.p);
      MG_HIP (hipGetLastError ());
      MG_HIP (hipStreamSynchronize (st));
      if (mgTextOutFromDevice (w, b->text.p, bytes)) { mgSetError ("failed to copy or write the report text"); return MG_ERR_HIP; }
    }
  return MG_OK;
}

extern "C" void mgRefPaintScratchFree (void *scratch) { delete (MgReportBufs *) scratch; }

/* modutils.c:262-270 for every record of a batch that is on the device: scan + lookups with positions (mgSeedsOfBatch: the
   seeds in (read, pos) order, misses included), the headers and seed lines put in one order, formatted, handed to the writer */
extern "C" int mgRefPaintBatchDevice (Modset *ms, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                      const char *idBytes, const U64 *idOff, MgTextOut *w, void **scratch)
{
  if (!nReads) return 0;
  if (nReads >= MG_HDR_BIT) { mgSetError ("mgRefPaint: %u records in one batch (at most 2^31 - 1)", nReads); return -1; }
  if (!*scratch) *scratch = new MgReportBufs ();
  MgReportBufs *b = (MgReportBufs *) *scratch;
  hipStream_t st = 0;
  const char *const what = "mgRefPaint";
  const int wdt = ms && ms->hasher && ms->hasher->w > 0 ? ms->hasher->w : 1;
  U64 cap = totalBases / (U64) wdt * 2 + 4096, n = 0;
  if (cap > totalBases + 16) cap = totalBases + 16;
  if (mgSeedsOfBatch (ms, 0, 0, dPacked, totalBases, dReadOffsets, nReads, cap, &b->seeds, &n, (void *) st)) return -1;
  if (n + nReads >= ((U64) 1 << 32)) { mgSetError ("mgRefPaint: %llu lines in one batch", (unsigned long long) (n + nReads)); return -1; }
  const U64 *dValue1; const U16 *dDepth1; U32 max;
  if (mgHookDeviceView (ms, &dValue1, &dDepth1, &max)) { mgSetError ("mgRefPaint: the set's device view is not available"); return -1; }
  /* the batch's ids as one buffer: they are contiguous, record r's at idOff[r], each 0-terminated */
  const size_t idBytesLen = (size_t) idOff[nReads - 1] + strlen (idBytes + idOff[nReads - 1]) + 1;
  if (b->ids.reserve (idBytesLen, mgRoomFor (idBytesLen), what) || b->idOff.reserve (nReads, mgRoomFor (nReads), what)
      || b->start.reserve ((size_t) nReads + 1, mgRoomFor ((size_t) nReads + 1), what) || b->item.reserve (n + nReads, mgRoomFor (n + nReads), what)) return -1;
  if (hipMemcpyAsync (b->ids.p, idBytes, idBytesLen, hipMemcpyHostToDevice, st) != hipSuccess
      || hipMemcpyAsync (b->idOff.p, idOff, (size_t) nReads * 8, hipMemcpyHostToDevice, st) != hipSuccess)
    { mgHipFail (hipGetLastError (), "mgRefPaint: ids to the device"); return -1; }
  MG_LAUNCH (MG_K_PAINT_ITEMS, st, mgPaintStartKernel, dim3 (mgGrid (n + 1)), dim3 (256), 0, st, b->seeds.rid, n, nReads, b->start.p);
  MG_LAUNCH (MG_K_PAINT_ITEMS, st, mgPaintItemsKernel, dim3 (mgGrid (n + nReads)), dim3 (256), 0, st, b->seeds.rid, n, nReads, b->start.p, b->item.p);
  if (hipGetLastError () != hipSuccess) { mgSetError ("mgRefPaint: kernel launch failed"); return -1; }
  MgPaintLines L;
  L.item = b->item.p; L.seedIx = b->seeds.ix; L.seedPosF = b->seeds.posF; L.depth1 = dDepth1; L.readOff = dReadOffsets; L.ids = b->ids.p; L.idOff = b->idOff.p;
  return mgTextFormat (L, n + nReads, b, w, st) ? -1 : 0;
}

/* the body of mgReportDepths: entries 1 .. max of the set, a chunk at a time, to the writer */
static int mgReportDepthsTo (MgTextOut *w, Modset *ms, Modset **others, int nOthers, const U64 *dValue1, const U16 *dDepth1, U32 max,
                             const std::vector<const U16 *> &oDepth, const std::vector<int> &oBits)
{
  hipStream_t st = 0;
  MgReportBufs b;
  MgDevScratch scratch ("mgReportDepths");
  U8 *dInfo; U64 *dKey; U32 *dIdx; U16 *dOth;
  const U64 chunk = max < MG_TEXT_CHUNK ? max : MG_TEXT_CHUNK;
  if (scratch.get (&dInfo, max) || scratch.get (&dKey, chunk) || scratch.get (&dIdx, chunk) || scratch.get (&dOth, (nOthers ? nOthers : 1) * chunk)) return -1;
  if (mgCopyH2DBig (dInfo, ms->info + 1, max)) return -1;                /* msCopy: the host info[] is the authority */
  for (U64 i0 = 0 ; i0 < max ; i0 += chunk)
    { const U64 m = max - i0 < chunk ? max - i0 : chunk;
      for (int o = 0 ; o < nOthers ; ++o)
        { MG_LAUNCH (MG_K_DEPTH_GUARD, st, mgDepthGuardKernel, dim3 (mgGrid (m)), dim3 (256), 0, st, dValue1 + i0, m, oBits[o], dKey);
          if (modsetFindBatchDevice (others[o], dKey, m, dIdx, (void *) st)) return -1;
          MG_LAUNCH (MG_K_DEPTH_GATHER, st, mgDepthGatherKernel, dim3 (mgGrid (m)), dim3 (256), 0, st, dValue1 + i0, m, oBits[o], dIdx, oDepth[o], dOth + (U64) o * m);
        }
      MgDepthLines L;
      L.value = dValue1 + i0; L.depth = dDepth1 + i0; L.info = dInfo + i0; L.oth = dOth; L.nOth = nOthers; L.m = m;
      if (mgTextFormat (L, m, &b, w, st)) return -1;
    }
  return 0;
}

/* modutils.c:65-77.  The other sets' device tables are made on first use (from their host arrays) and left resident: the caller
   releases them with mgModsetDeviceRelease or modsetDestroy. */
extern "C" int mgReportDepths (Modset *ms, Modset **others, int nOthers, FILE *f)
{
  if (!ms || !ms->hasher || !f || nOthers < 0 || (nOthers && !others)) { mgSetError ("mgReportDepths: invalid arguments"); return -1; }
  for (int o = 0 ; o < nOthers ; ++o) if (!others[o] || !others[o]->hasher) { mgSetError ("mgReportDepths: other set %d is null", o); return -1; }
  if (mgEnsureDevice ()) return -1;
  const U64 *dValue1; const U16 *dDepth1; U32 max;
  if (mgHookDeviceViewMake (ms, &dValue1, &dDepth1, &max)) { if (!mgLastError ()[0]) mgSetError ("mgReportDepths: no device view of the set"); return -1; }
  std::vector<const U16 *> oDepth (nOthers); std::vector<int> oBits (nOthers);
  for (int o = 0 ; o < nOthers ; ++o)
    { const U64 *v; U32 m;
      if (mgHookDeviceViewMake (others[o], &v, &oDepth[o], &m)) { if (!mgLastError ()[0]) mgSetError ("mgReportDepths: no device view of other set %d", o); return -1; }
      oBits[o] = 2 * others[o]->hasher->k;
    }
  if (!max) return 0;
  MgTextOut *w = mgTextOutOpen (f);                       /* closed on every path; a failed close is the error only if nothing failed before it */
  int rc = mgReportDepthsTo (w, ms, others, nOthers, dValue1, dDepth1, max, oDepth, oBits);
  if (mgTextOutClose (w) && !rc) { mgSetError ("mgReportDepths: write failed"); rc = -1; }
  return rc;
}

static int mgModsetWriteTextTo (MgTextOut *w, Modset *ms, const U64 *dValue1, const U16 *dDepth1, U32 max)
{
  MgReportBufs b;
  MgDevScratch scratch ("mgModsetWriteTextDevice");
  U8 *dInfo;
  if (scratch.get (&dInfo, max)) return -1;
  if (mgCopyH2DBig (dInfo, ms->info + 1, max)) return -1;                /* the host info[] is the authority */
  MgSetLines L;
  L.value = dValue1; L.depth = dDepth1; L.info = dInfo; L.k = ms->hasher->k;
  return mgTextFormat (L, (U64) max, &b, w, 0) ? -1 : 0;
}

/* modutils.c:191-199.  The header line is the host's, written before the writer thread exists, so the bytes are in order. */
extern "C" int mgModsetWriteTextDevice (Modset *ms, FILE *f)
{
  if (!ms || !ms->hasher || !f) { mgSetError ("mgModsetWriteTextDevice: invalid arguments"); return -1; }
  if (mgEnsureDevice ()) return -1;
  const Seqhash *sh = ms->hasher;
  if (!mgHookHasDevice (ms) && sh->k < 32)               /* a set from the host: no value of 4^k or more may enter a device table (mgDepthGuardKernel) */
    for (U32 i = 1 ; i <= ms->max ; ++i)
      if (ms->value[i] >> (2 * sh->k)) { mgSetError ("mgModsetWriteTextDevice: entry %u holds a value of 4^k or more (mgModsetWriteText writes such a set)", i); return -1; }
  const U64 *dValue1; const U16 *dDepth1; U32 max;
  if (mgHookDeviceViewMake (ms, &dValue1, &dDepth1, &max)) { if (!mgLastError ()[0]) mgSetError ("mgModsetWriteTextDevice: no device view of the set"); return -1; }
  if (fprintf (f, "modset bits %d size %d k %d w %d seed %d\n", ms->tableBits, max + 1, sh->k, sh->w, sh->seed) < 0)
    { mgSetError ("mgModsetWriteTextDevice: write failed"); return -1; }
  if (!max) return 0;
  MgTextOut *w = mgTextOutOpen (f);
  int rc = mgModsetWriteTextTo (w, ms, dValue1, dDepth1, max);
  if (mgTextOutClose (w) && !rc) { mgSetError ("mgModsetWriteTextDevice: write failed"); rc = -1; }
  return rc;
}
