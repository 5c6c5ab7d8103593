/* mg_gunzip.hip — ordinary gzip inflated on the device: the kernels (gfx950, wave64), the batch that launches them (MgGunzipDev), and the host compile
 * of the same pipeline (mgGunzipHost).  The arithmetic of every stage is mg_gunzip_core.h, written once for both sides; the stream above the batches
 * (members, headers, trailers, the capacity retries: mgzNext) is that file's too, so the two compiles count the same chunks in mgGunzipDiag.
 *
 * WHY THE TEXT IS RIGHT.  Chunk 0 of a batch starts at a true block start (the first bit behind a member's header, or where the chunk confirmed last
 * ended).  Chunk i + 1 is confirmed if and only if chunk i is confirmed and its decode ended exactly on chunk i + 1's candidate.  A decode from a true
 * block start ends on true block boundaries only, so by induction every confirmed start is a true block start and every confirmed chunk's symbols are
 * what a serial decoder produces there; what a false candidate decoded is never looked at.  The first chunk that breaks the chain ends the batch, and
 * the next one starts at the end of the last confirmed chunk with the window in hand: every batch confirms at least its first chunk.
 *
 * A batch is four launches on the caller's stream:
 *   find     one wave a chunk.  A step tests 64 consecutive bit offsets, one a lane, each from two unaligned 8-byte loads (mgzCheap: registers only);
 *            the ballot's survivors are verified one at a time in ascending order, wave-uniform, by lane 0 on the wave's LDS tables (mgzVerify).
 *   decode   one wave a workgroup and chunk, the tables (MgInfTables, 4608 bytes) in LDS, lane 0 decoding (mgzChunkDecode) into the chunk's own stretch
 *            of 16-bit symbols -- as in mg_inflate.hip a match is read and written by the same lane in program order.
 *   chain    ONE workgroup of 1024 walks the confirmed chunks in order: thread 0 takes the step (mgzChainStep: confirmation, the text offsets -- the
 *            exclusive scan of the confirmed lengths falls out of the walk), all threads then write the 32 KiB window behind the chunk
 *            (mgzWindowSym), a barrier between the steps.  Serial in chunks, parallel within the window.
 *   resolve  a workgroup per 16 Ki symbols of a confirmed chunk: symbols and the window before the chunk become bytes, each thread's CRC-32 is shifted
 *            to the tile's end, xor-ed across the workgroup, shifted to the batch's end and xor-ed into the batch's CRC.
 * Then the summary (96 bytes) comes back and the host decides where the next batch starts.  Stores to memory are the compiler's vector stores: plain C++. */
#include <string.h>
#include <unistd.h>
#include <vector>
#include "mg_common.h"
#include "mg_internal.h"
#include "mg_gunzip_core.h"

#define GZ_CHAIN_THREADS 1024
#define GZ_RES_THREADS 256
#define GZ_RES_PER 64u                                   /* symbols a thread resolves */
#define GZ_RES_TILE (GZ_RES_THREADS * GZ_RES_PER)

__global__ __launch_bounds__ (64)
void mgGunzipFindKernel (const U8 *__restrict__ comp, U64 n, U64 start, U32 chunkBytes, U32 nChunks, MgzChunk *__restrict__ ch)
{
  __shared__ MgInfTables T;
  const U32 c = blockIdx.x, lane = threadIdx.x;
  if (c >= nChunks) return;
  U64 cand = MGZ_NONE;
  if (!c) cand = start;
  else
    { U64 lo, hi;
      mgzChunkRange (start, chunkBytes, c, n, &lo, &hi);
      for (U64 p0 = lo ; p0 < hi && cand == MGZ_NONE ; p0 += 64)
        { const U64 p = p0 + lane;
          unsigned long long mask = __ballot (p < hi && mgzCheapAt (comp, n, p));
          while (mask)
            { const U32 k = (U32) __ffsll ((long long) mask) - 1;
              mask &= mask - 1;
              int v = 0;
              if (lane == 0) v = mgzVerify (comp, n, p0 + k, &T);
              v = __shfl (v, 0);
              if (v) { cand = p0 + k; break; }
            }
        }
    }
  if (lane == 0)
    { MgzChunk k; k.cand = cand; k.end = 0; k.off = 0; k.nSym = 0; k.status = 0; k.final = 0; k.ok = 0; k.wlen = 0; k.pad = 0;
      ch[c] = k;
    }
}

__global__ __launch_bounds__ (64)
void mgGunzipDecodeKernel (const U8 *__restrict__ comp, U64 n, MgzChunk *ch, U32 nChunks, U64 batchEnd, uint16_t *sym, U32 cap, U32 wlen)
{
  __shared__ MgInfTables T;
  const U32 c = blockIdx.x;
  if (c >= nChunks || threadIdx.x) return;
  const U64 cand = ch[c].cand;
  if (cand == MGZ_NONE) return;
  U64 end = 0; U32 nSym = 0, final = 0;
  const U32 st = mgzChunkDecode (comp, n, cand, mgzStopOf (ch, nChunks, c, batchEnd), c ? ~(U32) 0 : wlen, sym + (size_t) c * cap, cap, &T, &end, &nSym, &final);
  ch[c].end = end; ch[c].nSym = nSym; ch[c].final = final; ch[c].status = st;
}

__global__ __launch_bounds__ (GZ_CHAIN_THREADS)
void mgGunzipChainKernel (MgzChunk *ch, U32 nChunks, const uint16_t *__restrict__ sym, U32 cap, U8 *win, U64 start, U32 wlen, U64 outCap, MgzSummary *out)
{
  __shared__ MgzSummary S;
  __shared__ U32 next, slot, ok, nSym;
  const U32 t = threadIdx.x;
  if (!t) mgzChainBegin (&S, start, wlen);
  __syncthreads ();
  for (U32 c = 0 ; c < nChunks ; )
    { if (!t) { next = mgzChainStep (ch, nChunks, c, outCap, &S); slot = (U32) S.carrySlot; ok = ch[c].ok; nSym = ch[c].nSym; }
      __syncthreads ();                                  /* the step's verdict; the window the step before wrote */
      if (ok)
        { const U8 *before = win + (size_t) c * MGZ_WINDOW;
          U8 *after = win + (size_t) slot * MGZ_WINDOW;
          const uint16_t *s = sym + (size_t) c * cap;
          for (U32 j = t ; j < MGZ_WINDOW ; j += GZ_CHAIN_THREADS) after[j] = mgzWindowSym (before, s, nSym, j);
        }
      const U32 nx = next;
      __syncthreads ();
      c = nx;
    }
  if (!t) *out = S;
}

__global__ __launch_bounds__ (GZ_RES_THREADS)
void mgGunzipResolveKernel (const MgzChunk *__restrict__ ch, U32 nChunks, const uint16_t *__restrict__ sym, U32 cap, const U8 *__restrict__ win, U8 *text, MgzSummary *S)
{
  __shared__ uint32_t tab[256];
  __shared__ U32 part[GZ_RES_THREADS / 64];
  const U32 c = blockIdx.x, t = threadIdx.x;
  if (c >= nChunks) return;
  const MgzChunk k = ch[c];
  const U64 tile0 = (U64) blockIdx.y * GZ_RES_TILE;
  if (!k.ok || tile0 >= k.nSym) return;                  /* (uniform over the workgroup) */
  mgInfCrcTable (tab, t, GZ_RES_THREADS);
  __syncthreads ();
  const U32 tileEnd = tile0 + GZ_RES_TILE < k.nSym ? (U32) tile0 + GZ_RES_TILE : k.nSym;
  U32 a = (U32) tile0 + t * GZ_RES_PER, e = a + GZ_RES_PER, bad = 0, crc = 0;
  if (a > tileEnd) a = tileEnd;
  if (e > tileEnd) e = tileEnd;
  if (a < e)
    { crc = mgzResolveSlice (tab, sym + (size_t) c * cap, win + (size_t) c * MGZ_WINDOW, k.wlen, a, e, text + k.off, &bad);
      if (e < tileEnd) crc = mgiMulModP (mgiXPow8 (tileEnd - e), crc);
    }
  for (int d = 32 ; d ; d >>= 1) crc ^= (U32) __shfl_xor ((int) crc, d);
  if (!(t & 63)) part[t >> 6] = crc;
  if (bad) atomicMin ((unsigned long long *) &S->badMarker, (unsigned long long) k.cand);
  __syncthreads ();
  if (!t)
    { U32 v = 0;
      for (U32 i = 0 ; i < GZ_RES_THREADS / 64 ; ++i) v ^= part[i];
      v = mgiMulModP (mgiXPow8 ((U32) (S->outBytes - k.off - tileEnd)), v);
      atomicXor ((unsigned long long *) &S->crc, (unsigned long long) v);
    }
}

/* ---------------------------------------------------------------------------------------------------------------- the calling thread's census */
static thread_local U64 gGzDiag[8];
extern "C" void mgGunzipDiag (U64 out8[8]) { memcpy (out8, gGzDiag, sizeof (gGzDiag)); }
extern "C" void mgGunzipDiagReset (void) { memset (gGzDiag, 0, sizeof (gGzDiag)); }

/* ---------------------------------------------------------------------------------------------------------------- a stream on the device */
struct MgGunzipDev {
  const U8 *dComp = 0; U64 n = 0; int fd = -1;
  U32 chunkBytes = 0, batchChunks = 0, spc = 0;
  MgzStream st;
  U64 reported[8];
  hipStream_t stream = 0;
  MgDevBuf<MgzChunk> ch; MgDevBuf<uint16_t> sym; MgDevBuf<U8> win, text;
  U8 *dCarry = 0; MgzSummary *dSum = 0, *hSum = 0;
  bool hipFailed = false;
  MgGunzipRangeFn range = 0; void *rangeCtx = 0;         /* one walk: who keeps the part of the file that is on the device */
};

static uint32_t gzDevPeek (void *v, uint64_t off, uint8_t *buf, uint32_t n)
{
  MgGunzipDev *g = (MgGunzipDev *) v;
  uint32_t got = 0;
  while (got < n)
    { const ssize_t r = pread (g->fd, buf + got, n - got, (off_t) (off + got));
      if (r <= 0) break;
      got += (uint32_t) r;
    }
  return got;
}
/* one run of plan P over comp[.. n) -- the whole file, or a resident range of it by a pointer biased by the range's first offset: every kernel reads at
   P->start's byte or behind it, and below n */
static bool gzDevRun (MgGunzipDev *g, const MgzPlan *P, const U8 *comp, U64 n, size_t nSym)
{
  hipStream_t st = g->stream;
  U64 lo, batchEnd;
  mgzChunkRange (P->start, P->chunkBytes, P->nChunks - 1, n, &lo, &batchEnd);
  const U32 tiles = (U32) (((U64) P->cap + GZ_RES_TILE - 1) / GZ_RES_TILE);
  if (hipMemcpyAsync (g->win.p, g->dCarry, MGZ_WINDOW, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
  hipLaunchKernelGGL (mgGunzipFindKernel, dim3 (P->nChunks), dim3 (64), 0, st, comp, n, P->start, P->chunkBytes, P->nChunks, g->ch.p);
  hipLaunchKernelGGL (mgGunzipDecodeKernel, dim3 (P->nChunks), dim3 (64), 0, st, comp, n, g->ch.p, P->nChunks, batchEnd, g->sym.p, P->cap, P->wlen);
  hipLaunchKernelGGL (mgGunzipChainKernel, dim3 (1), dim3 (GZ_CHAIN_THREADS), 0, st, g->ch.p, P->nChunks, g->sym.p, P->cap, g->win.p, P->start, P->wlen, (U64) nSym, g->dSum);
  hipLaunchKernelGGL (mgGunzipResolveKernel, dim3 (P->nChunks, tiles), dim3 (GZ_RES_THREADS), 0, st, g->ch.p, P->nChunks, g->sym.p, P->cap, g->win.p, g->text.p, g->dSum);
  return hipGetLastError () == hipSuccess
         && hipMemcpyAsync (g->hSum, g->dSum, sizeof (MgzSummary), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize (st) == hipSuccess;
}
static int gzDevBatch (void *v, const MgzPlan *P, MgzSummary *S)
{
  MgGunzipDev *g = (MgGunzipDev *) v;
  hipStream_t st = g->stream;
  const char *what = "gzip on the device";
  const size_t nSym = (size_t) P->nChunks * P->cap;
  if (g->ch.reserve (P->nChunks, P->nChunks, what) || g->sym.reserve (nSym, nSym, what) || g->text.reserve (nSym, nSym, what)
      || g->win.reserve (((size_t) P->nChunks + 1) * MGZ_WINDOW, ((size_t) P->nChunks + 1) * MGZ_WINDOW, what)) { g->hipFailed = true; return -1; }
  bool ok;
  if (!g->range) ok = gzDevRun (g, P, g->dComp, g->n, nSym);
  else
    /* One walk.  The batch's chunks and one more (the last chunk decodes on to a block boundary) are asked for; the range's owner says what is there.
       A decode that runs out of resident bytes before the file's end says nothing about the stream: behind confirmed chunks it ends the chain like a
       broken one (the next batch starts at that chunk, with more bytes resident); in chunk 0 -- a stored block of 65 535 bytes, a long dynamic block
       against a range of a few KiB -- the range grows and the batch is run again.  Only at the file's true end is it the stream's error */
    for (U64 span = ((U64) P->nChunks + 1) * P->chunkBytes ; ; span *= 2)
      { const U64 lo = P->start >> 3, hi = g->n - lo < span ? g->n : lo + span;
        const U8 *comp = 0; U64 n = 0;
        if (g->range (g->rangeCtx, lo, hi, (void *) st, &comp, &n)) { g->hipFailed = true; return -1; }
        if (n < hi || n > g->n) { mgSetError ("gzip on the device: bytes %llu .. %llu asked for, the range ends at %llu", (unsigned long long) lo, (unsigned long long) hi, (unsigned long long) n); g->hipFailed = true; return -1; }
        if (!(ok = gzDevRun (g, P, comp, n, nSym))) break;
        MgzSummary *h = g->hSum;
        if (n == g->n || h->reason != MGZ_ERROR || h->status != MGI_INPUT) break;
        if (h->confirmed) { h->reason = MGZ_BROKE; break; }
      }
  if (ok)
    { *S = *g->hSum;
      if (S->carrySlot > P->nChunks) { mgSetError ("gzip on the device: the chain's summary is not of this batch"); return -1; }
      ok = hipMemcpyAsync (g->dCarry, g->win.p + (size_t) S->carrySlot * MGZ_WINDOW, MGZ_WINDOW, hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
  if (!ok) { mgHipFail (hipGetLastError (), what); g->hipFailed = true; return -1; }
  return 0;
}

static void gzDevRestart (MgGunzipDev *g)
{ mgzStreamInit (&g->st, g->n, g->chunkBytes, g->batchChunks, g->spc, ~(U64) 0); memset (g->reported, 0, sizeof (g->reported)); }

extern "C" int mgGunzipDevOpen (const U8 *dComp, U64 n, int fd, U32 chunkBytes, U32 batchChunks, U32 symbolsPerChunk, MgGunzipDev **out)
{
  *out = 0;
  MgGunzipDev *g = new MgGunzipDev;
  g->dComp = dComp; g->n = n; g->fd = fd; g->chunkBytes = chunkBytes; g->batchChunks = batchChunks; g->spc = symbolsPerChunk;
  gzDevRestart (g);
  g->hSum = (MgzSummary *) mgPinnedAlloc (sizeof (MgzSummary));
  if (!g->hSum || hipMalloc ((void **) &g->dCarry, MGZ_WINDOW) != hipSuccess || hipMalloc ((void **) &g->dSum, sizeof (MgzSummary)) != hipSuccess
      || hipMemset (g->dCarry, 0, MGZ_WINDOW) != hipSuccess)
    { mgHipFail (hipGetLastError (), "gzip on the device"); mgGunzipDevClose (g); return -1; }
  *out = g;
  return 0;
}
extern "C" void mgGunzipDevClose (MgGunzipDev *g)
{
  if (!g) return;
  g->ch.drop (); g->sym.drop (); g->win.drop (); g->text.drop ();
  (void) hipFree (g->dCarry); (void) hipFree (g->dSum); mgPinnedFree (g->hSum);
  delete g;
}
extern "C" void mgGunzipDevRewind (MgGunzipDev *g) { gzDevRestart (g); }
extern "C" void mgGunzipDevRange (MgGunzipDev *g, MgGunzipRangeFn fn, void *ctx) { g->range = fn; g->rangeCtx = ctx; }

/* the stream's next text: batches on `stream` until one has text or the stream ends.  *dText holds *n bytes until the next call.  0; -1 with
   mgLastError: the stream is wrong (*status and the compressed byte *errOff say where), or the device failed (*status 0) */
extern "C" int mgGunzipDevNext (MgGunzipDev *g, void *stream, const U8 **dText, size_t *n, int *done, U32 *status, U64 *errOff)
{
  *dText = 0; *n = 0; *status = 0; *errOff = 0;
  g->stream = (hipStream_t) stream;
  int rc = 0;
  while (!g->st.done)
    { const U64 before = g->st.produced;
      rc = mgzNext (&g->st, gzDevPeek, gzDevBatch, g);
      for (int i = 0 ; i < 8 ; ++i) { gGzDiag[i] += g->st.diag[i] - g->reported[i]; g->reported[i] = g->st.diag[i]; }
      if (g->st.produced > before) { *dText = g->text.p; *n = (size_t) (g->st.produced - before); }
      if (rc || *n) break;
    }
  *done = g->st.done;
  if (rc == -1) { *status = g->st.status; *errOff = g->st.errOff; }
  return rc ? -1 : 0;
}

/* ---------------------------------------------------------------------------------------------------------------- the host compile */
struct GzHost { MgzHostMem M; std::vector<MgzChunk> ch; std::vector<uint16_t> sym; std::vector<uint8_t> win; uint8_t *out; uint64_t produced; MgInfTables T; };

static uint32_t gzHostPeek (void *v, uint64_t off, uint8_t *buf, uint32_t n)
{
  const GzHost *h = (const GzHost *) v;
  if (off >= h->M.n) return 0;
  if (h->M.n - off < n) n = (uint32_t) (h->M.n - off);
  memcpy (buf, h->M.comp + off, n);
  return n;
}
static int gzHostBatch (void *v, const MgzPlan *P, MgzSummary *S)
{
  GzHost *h = (GzHost *) v;
  const size_t nSym = (size_t) P->nChunks * P->cap;
  try
    { if (h->ch.size () < P->nChunks) h->ch.resize (P->nChunks);
      if (h->sym.size () < nSym) h->sym.resize (nSym);
      if (h->win.size () < ((size_t) P->nChunks + 1) * MGZ_WINDOW) h->win.resize (((size_t) P->nChunks + 1) * MGZ_WINDOW);
    }
  catch (...) { mgSetError ("mgGunzipHost: no memory for %zu symbols", nSym); return -1; }
  h->M.ch = h->ch.data (); h->M.sym = h->sym.data (); h->M.win = h->win.data (); h->M.out = h->out + h->produced; h->M.T = &h->T;
  mgzBatchHost (&h->M, P, S);
  h->produced += S->outBytes;
  return 0;
}

/* the same pipeline on the calling thread: the CPU tests' subject and the GPU tests' yardstick */
extern "C" int mgGunzipHost (const U8 *comp, U64 n, U32 chunkBytes, U32 batchChunks, U32 symbolsPerChunk, U8 *out, U64 cap, U64 *outLen, U32 *status, U64 diag8[8])
{
  if (outLen) *outLen = 0;
  if (status) *status = 0;
  if (diag8) memset (diag8, 0, 8 * sizeof (U64));
  if ((!comp && n) || (!out && cap)) { mgSetError ("mgGunzipHost: null argument"); return -1; }
  GzHost h; h.M.comp = comp; h.M.n = n; h.out = out; h.produced = 0;
  MgzStream st;
  mgzStreamInit (&st, n, chunkBytes, batchChunks, symbolsPerChunk, cap);
  int rc = 0;
  while (!st.done && !rc) rc = mgzNext (&st, gzHostPeek, gzHostBatch, &h);
  if (rc == -2) return -1;
  if (outLen) *outLen = st.produced;
  if (status) *status = st.status;
  if (diag8) memcpy (diag8, st.diag, sizeof (st.diag));
  return 0;
}
