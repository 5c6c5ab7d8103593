/* mg_textwin.hip — the device text parser's windows: the buffers of every device, the file mover, the window sources and the ONE walk over the two
 * buffers that the parse loop (mg_textparse.hip) and the window streamer for composition and seqconvert (mgTextStreamWindows, below) are written over. */
#include <stdlib.h>
#include <unistd.h>
#include <thread>
#include "mg_text_int.h"

void TxBufs::release ()
{
  for (int i = 0 ; i < 2 ; ++i)
    { if (hPin[i]) (void) hipHostFree (hPin[i]);
      if (h2dDone[i]) (void) hipEventDestroy (h2dDone[i]);
      (void) hipFree (dText[i]); hPin[i] = 0; h2dDone[i] = 0; dText[i] = 0;
    }
  if (copy) (void) hipStreamDestroy (copy);
  if (hCounts) (void) hipHostFree (hCounts);
  copy = 0; hCounts = 0;
  dState.drop (); dTq.drop (); dOverflow.drop (); dOpenLine.drop ();
  dTileEvent.drop (); dTileBaseOff.drop (); dTileStartOff.drop (); dTileOffQ.drop (); dTileBases.drop (); dTileStarts.drop (); dTileQual.drop ();
  dBases.drop (); dRecOff.drop (); dEndQ.drop (); dEndP.drop (); dRecPos.drop (); dPacked.drop ();
  hHdr.drop (); dIdLen.drop (); dIdLenT.drop (); dIdPlace.drop (); dIdBytes.drop (); hIdBytes.drop (); hIdPlace.drop ();
  basesCap = recCap = window = 0; dev = -1;
}
TxBufs gTxs[TX_MAXDEV];
extern "C" void mgTextReleaseBuffers (void)
{
  int before = -1; if (hipGetDevice (&before) != hipSuccess) { (void) hipGetLastError (); before = -1; }
  for (int dev = 0 ; dev < TX_MAXDEV ; ++dev)
    { std::lock_guard<std::mutex> g (gTxs[dev].lock);
      if (gTxs[dev].dev >= 0) { (void) hipSetDevice (gTxs[dev].dev); gTxs[dev].release (); }
    }
  if (before >= 0) (void) hipSetDevice (before);
}

int txReserve (TxBufs &t, size_t window, U64 basesNeed, U64 recsNeed)
{
  int dev = 0; if (hipGetDevice (&dev) != hipSuccess) return -1;
  if (t.dev >= 0 && (t.dev != dev || t.window < window)) t.release ();      /* (buffers made for a larger window serve a smaller one) */
  const char *what = "device text parser";
  bool ok = true;
  if (t.dev < 0)
    { const size_t tiles = window / TX_TILE + 2;
      for (int i = 0 ; ok && i < 2 ; ++i)
        ok = hipHostMalloc ((void **) &t.hPin[i], window + 64, hipHostMallocDefault) == hipSuccess
             && hipEventCreateWithFlags (&t.h2dDone[i], hipEventDisableTiming) == hipSuccess && hipMalloc ((void **) &t.dText[i], window + 64) == hipSuccess;
      ok = ok && hipHostMalloc ((void **) &t.hCounts, 64, hipHostMallocDefault) == hipSuccess && hipStreamCreateWithFlags (&t.copy, hipStreamNonBlocking) == hipSuccess
           && !t.dState.reserve (1, 1, what) && !t.dTq.reserve (1, 1, what) && !t.dOverflow.reserve (1, 1, what) && !t.dOpenLine.reserve (1, 1, what)
           && !t.dTileEvent.reserve (tiles, tiles, what) && !t.dTileBaseOff.reserve (tiles, tiles, what) && !t.dTileStartOff.reserve (tiles, tiles, what)
           && !t.dTileOffQ.reserve (tiles, tiles, what) && !t.dTileBases.reserve (tiles, tiles, what) && !t.dTileStarts.reserve (tiles, tiles, what)
           && !t.dTileQual.reserve (tiles, tiles, what);
      if (ok) { t.dev = dev; t.window = window; }
    }
  if (ok && basesNeed > t.basesCap)
    { size_t cap = (size_t) (basesNeed + basesNeed / 4 + (1 << 20)); if (cap < 2 * t.basesCap) cap = 2 * t.basesCap;
      if ((ok = t.dBases.grow (t.basesCap, cap))) t.basesCap = cap;
    }
  if (ok && recsNeed > t.recCap)
    { size_t cap = (size_t) (recsNeed + recsNeed / 4 + 4096); if (cap < 2 * t.recCap) cap = 2 * t.recCap;
      if ((ok = t.dRecOff.grow (t.recCap, cap) && t.dEndQ.grow (t.recCap, cap) && t.dEndP.grow (t.recCap, cap) && t.dRecPos.grow (t.recCap, cap))) t.recCap = cap;
    }
  if (!ok) t.release ();      /* an allocation failed half way: everything is given back */
  return ok ? 0 : -1;
}

/* text per window: 128 MiB (two pinned and two device buffers of that size are kept between calls; 64 MiB windows: 31.6 Gbp/s on a
   4 Gbp file, 256 MiB: 34.8), less for a file that is smaller */
size_t txWindowBytes (size_t fileSize)
{
  const long wk = mgKnobs ()->textWindowKb;                  /* test knob: small windows put window and batch edges everywhere */
  long kb = wk != MG_KNOB_UNSET ? wk : 0;
  size_t w = kb > 0 ? (size_t) kb << 10 : (size_t) 128 << 20;
  if (kb <= 0) while (w > ((size_t) 1 << 20) && w / 2 >= fileSize) w /= 2;
  return (w + TX_TILE - 1) / TX_TILE * TX_TILE;
}
U64 txBatchBases (U64 asked)
{
  const MgKnobs *kn = mgKnobs ();
  long mbp = kn->fileBatchMbp != MG_KNOB_UNSET ? kn->fileBatchMbp : 1024;
  if (mbp < 1) mbp = 1;
  U64 b = (U64) mbp * 1000000;
  if (asked && kn->fileBatchMbp == MG_KNOB_UNSET) b = asked;
  if (kn->fileBatchBases != MG_KNOB_UNSET && kn->fileBatchBases > 0) b = (U64) kn->fileBatchBases;        /* test knob (as in mg_seqio.c) */
  return b;
}

/* [off, off + n) of the file into dst, by a team of threads (the copy out of the page cache is the cost) */
static bool txReadParallel (int fd, unsigned char *dst, size_t n, off_t off, int nThreads)
{
  if (nThreads < 1) nThreads = 1;
  const size_t slice = ((n + nThreads - 1) / nThreads + 4095) & ~(size_t) 4095;
  volatile int bad = 0;
  auto work = [&] (int t)
    { size_t a = slice * (size_t) t, b = a + slice < n ? a + slice : n;
      while (a < b)
        { ssize_t g = pread (fd, dst + a, b - a, off + (off_t) a);
          if (g <= 0) { bad = 1; return; }
          a += (size_t) g;
        }
    };
  std::vector<std::thread> th;
  int started = 1;
  try { for (int t = 1 ; t < nThreads && slice * (size_t) t < n ; ++t) { th.emplace_back (work, t); ++started; } }
  catch (...) { }
  work (0);
  for (auto &x : th) x.join ();
  for (int t = started ; t < nThreads && slice * (size_t) t < n ; ++t) work (t);      /* threads that could not be started */
  return !bad;
}
int txHostThreads (void)
{
  const long pk = mgKnobs ()->parseThreads;
  long v = pk != MG_KNOB_UNSET ? pk : 0;
  if (v <= 0) v = mgCpuBudget ();
  if (v < 1) v = 1;
  if (v > 32) v = 32;
  return (int) v;
}
/* the two for mg_settext.hip (mg_internal.h) */
extern "C" int mgTextReadParallel (int fd, unsigned char *dst, size_t n, int64_t off) { return txReadParallel (fd, dst, n, (off_t) off, txHostThreads ()) ? 0 : -1; }
extern "C" size_t mgTextWindowBytes (size_t fileSize) { return txWindowBytes (fileSize); }

static size_t txPlainFill (void *v, unsigned char *dst, size_t cap, U64 off)
{
  const TxPlain *p = (const TxPlain *) v;
  if (off >= p->size) return 0;
  if (p->size - off < cap) cap = (size_t) (p->size - off);
  return txReadParallel (p->fd, dst, cap, (off_t) off, p->nThreads) ? cap : (size_t) -1;
}
TxSrc txSrcPlain (TxPlain *p) { TxSrc s; s.fill = txPlainFill; s.src = p; return s; }
static int txBgzfFill (void *v, unsigned char *dDst, size_t cap, U64 off, void *stream, size_t *n, int *more, U32 *first, U32 *last)
{ const TxBgzf *b = (const TxBgzf *) v; return mgBgzfSrcFill (b->bz, dDst, cap, off, b->size, stream, n, more, first, last); }
TxSrc txSrcBgzf (TxBgzf *b) { TxSrc s; s.dfill = txBgzfFill; s.src = b; return s; }
static int txGzipFill (void *v, unsigned char *dDst, size_t cap, U64 off, void *stream, size_t *n, int *more, U32 *first, U32 *last)
{ const TxGzip *z = (const TxGzip *) v; return mgGzipSrcFill (z->gz, dDst, cap, off, ~(U64) 0, stream, n, more, first, last); }      /* (no limit: the stream says where its text ends) */
TxSrc txSrcGzip (TxGzip *z) { TxSrc s; s.dfill = txGzipFill; s.src = z; return s; }

/* ---- the window walk (mg_text_int.h) ---- */
/* the window at `at` into buffer i and on its way */
int TxWalk::load (int i, U64 at, TxGot *o)
{
  *o = TxGot ();
  if (ck) ck->lap (ck->flush);
  if (src.dfill)
    { if (src.dfill (src.src, t.dText[i], window, at, (void *) t.copy, &o->n, &o->more, &o->first, &o->last)) return -1; }
  else
    { o->n = src.fill (src.src, t.hPin[i], window, at);
      if (o->n == (size_t) -1) { o->n = 0; mgSetError ("device text windows: read failed"); return -1; }
      o->more = o->n == window;
      if (o->n) { o->first = t.hPin[i][0]; o->last = t.hPin[i][o->n - 1]; }
      if (o->n && hipMemcpyAsync (t.dText[i], t.hPin[i], o->n, hipMemcpyHostToDevice, t.copy) != hipSuccess) return -2;
    }
  if (o->n && hipEventRecord (t.h2dDone[i], t.copy) != hipSuccess) return -2;
  if (ck) ck->lap (ck->read);
  return 0;
}
int TxWalk::start () { return load (0, 0, &got); }
int TxWalk::awaitCopy () { return hipStreamWaitEvent (st, t.h2dDone[cur ()], 0) == hipSuccess ? 0 : -2; }
int TxWalk::loadNext ()
{
  nxt = TxGot ();
  int rc = 0;
  if (got.more)                        /* (the other device buffer is free: its window's kernels were waited for) */
    { if (index >= 1 && hipEventSynchronize (t.h2dDone[cur () ^ 1]) != hipSuccess) return -2;
      rc = load (cur () ^ 1, off + got.n, &nxt);
    }
  eof = !nxt.n;
  return rc;
}
void TxWalk::advance () { prevByte = got.last; off += got.n; got = nxt; ++index; }
void TxWalk::drain () { (void) hipStreamSynchronize (t.copy); (void) hipStreamSynchronize (st); }

/* the window loop for a consumer that keeps nothing per base (mg_internal.h): the parser's buffers, its window size and its overlap of read,
   copy and kernels, without the batch accumulator */
static int txStreamWindows (size_t sizeHint, MgTextFillFn fill, MgTextDevFillFn dfill, void *src, MgTextWindowFn fn, void *ctx, U64 *nWindows)
{
  if (nWindows) *nWindows = 0;
  if (mgEnsureDevice ()) return -1;
  int curDev = 0;
  if (hipGetDevice (&curDev) != hipSuccess || curDev < 0 || curDev >= TX_MAXDEV) { (void) hipGetLastError (); mgSetError ("device text windows: no buffers are kept for this device"); return -1; }
  TxBufs &t = gTxs[curDev];
  std::lock_guard<std::mutex> g (t.lock);
  const size_t window = txWindowBytes (sizeHint);
  if (txReserve (t, window, 0, 0)) { mgSetError ("device text windows: allocation failed"); return -1; }
  TxSrc s; s.fill = fill; s.dfill = dfill; s.src = src;
  TxWalk wk (t, s, window, 0);
  int rc = wk.start ();
  if (rc == -1) return -1;
  while (wk.got.n && !rc)
    { if ((rc = wk.awaitCopy ())) break;
      MgTextWindow win; win.dText = wk.dText (); win.hText = wk.hText (); win.n = wk.got.n; win.off = wk.off; win.prevByte = wk.prevByte; win.index = wk.index;
      win.first = wk.got.first; win.last = wk.got.last;
      if (fn (ctx, &win, (void *) wk.st)) { rc = -1; break; }
      if ((rc = wk.loadNext ())) break;
      if (hipStreamSynchronize (wk.st) != hipSuccess) { rc = -2; break; }
      wk.advance ();
    }
  if (rc) wk.drain ();
  if (rc == -2) { mgSetError ("device text windows: HIP failure (%s)", hipGetErrorString (hipGetLastError ())); rc = -1; }
  if (nWindows) *nWindows = wk.index + (rc && wk.got.n ? 1 : 0);
  return rc;
}
extern "C" int mgTextStreamWindows (size_t sizeHint, MgTextFillFn fill, void *src, MgTextWindowFn fn, void *ctx, U64 *nWindows)
{ return txStreamWindows (sizeHint, fill, 0, src, fn, ctx, nWindows); }
extern "C" int mgTextStreamWindowsDev (size_t sizeHint, MgTextDevFillFn dfill, void *src, MgTextWindowFn fn, void *ctx, U64 *nWindows)
{ return txStreamWindows (sizeHint, 0, dfill, src, fn, ctx, nWindows); }
