/* mg_textids.hip — the record ids of the device text parser (TxIds, mg_text_int.h): cut out of the page-locked window by a team of host threads, or
 * out of the device's window by the id kernels; txWindowIds chooses. */
#include <pthread.h>
#include <string.h>
#include <thread>
#include "mg_text_int.h"

/* ---- the host team ---- */
void TxIds::feed (const unsigned char *p, size_t n)
{ if (skipOne) { if (!n) return; ++p; --n; skipOne = false; }
  size_t i = 0;
  while (i < n && !space (p[i])) ++i;
  bytes.insert (bytes.end (), (const char *) p, (const char *) p + i);
  if (i < n) { bytes.push_back (0); open = false; }
}
/* a header whose first byte ('>' / '@') is byte `at` of the window (at == n: the next window's first byte) */
void TxIds::header (const unsigned char *win, size_t n, size_t at)
{ off.push_back ((U64) bytes.size ()); open = true;
  if (at >= n) { skipOne = true; return; }
  feed (win + at + 1, n - at - 1);
}
/* cnt headers at window bytes at[0 .. cnt), every one of them with its id's end inside the window: lengths by a team of
   threads, places by a prefix over the threads' sums, copies by the team again (a window of short reads starts 4e5 records) */
void TxIds::headersTeam (const unsigned char *win, size_t n, const U64 *at, size_t cnt, int nThreads)
{ if (!cnt) return;
  if (nThreads > 16) nThreads = 16;
  if (cnt < 20000 || nThreads < 2) { for (size_t i = 0 ; i < cnt ; ++i) header (win, n, (size_t) at[i]); return; }
  std::vector<U32> len (cnt);
  std::vector<U64> sum ((size_t) nThreads + 1, 0);
  size_t base = 0, first = 0;
  pthread_barrier_t bar; pthread_barrier_init (&bar, 0, (unsigned) nThreads);
  /* one team for both passes (starting and joining fifteen threads costs as much as a pass): lengths; then member 0 makes the room; then copies */
  auto work = [&] (int t)
    { const size_t a = cnt * (size_t) t / nThreads, b = cnt * ((size_t) t + 1) / nThreads; U64 s = 0;
      for (size_t i = a ; i < b ; ++i)
        { if (i + 24 < b) __builtin_prefetch (win + at[i + 24] + 1);      /* a header per 300 bytes of a short-read file: every one is a cache miss */
          const unsigned char *p = win + at[i] + 1, *e = win + n; const unsigned char *q = p;
          while (q < e && !space (*q)) ++q;
          len[i] = (U32) (q - p); s += (U64) (q - p) + 1;
        }
      sum[(size_t) t + 1] = s;
      pthread_barrier_wait (&bar);
      if (t == 0)
        { for (int u = 0 ; u < nThreads ; ++u) sum[(size_t) u + 1] += sum[(size_t) u];
          base = bytes.size (); first = off.size ();
          bytes.resize (base + (size_t) sum[(size_t) nThreads]); off.resize (first + cnt);
        }
      pthread_barrier_wait (&bar);
      size_t o = base + (size_t) sum[(size_t) t];
      for (size_t i = a ; i < b ; ++i)
        { off[first + i] = (U64) o; memcpy (bytes.data () + o, win + at[i] + 1, len[i]); o += len[i]; bytes[o++] = 0; }
    };
  const double tA = mgNowS ();
  { std::vector<std::thread> th; for (int t = 1 ; t < nThreads ; ++t) th.emplace_back (work, t); work (0); for (auto &x : th) x.join (); }
  pthread_barrier_destroy (&bar);
  tLens += mgNowS () - tA;
  open = false;
}
/* the headers of a window: all but the last through the team (an id ends before the next header starts), the last one -- which may
   run on into the next window -- by header () */
void TxIds::headers (const unsigned char *win, size_t n, std::vector<U64> &at, int nThreads)
{ if (at.empty ()) return;
  const size_t cnt = at.size ();
  if (cnt > 1) headersTeam (win, n, at.data (), cnt - 1, nThreads);
  header (win, n, (size_t) at[cnt - 1]);
}
void TxIds::dropFront (size_t nRec)
{ if (!nRec) return;
  const U64 cut = nRec < off.size () ? off[nRec] : (U64) bytes.size ();
  bytes.erase (bytes.begin (), bytes.begin () + (ptrdiff_t) cut);
  off.erase (off.begin (), off.begin () + (ptrdiff_t) (nRec < off.size () ? nRec : off.size ()));
  for (auto &o : off) o -= cut;
}

/* ---- record ids on the device ----
 * For a window that has no page-locked copy (a device source), and for plain files under MODGPU_TEXT_IDS_DEVICE=1: the ids are cut out where
 * the text is.  Entry g of a window is an id that starts at byte start (g): the byte after a header's first byte -- the emit kernels' recPos
 * (FASTA) or endP + 1 (FASTQ) say where the headers are -- or, for the one explicit entry in front (nPre), the continuation of an id the
 * window before left open (byte 0, or 1 when that header's first byte is this window's first: TxIds::skipOne) or the FASTQ header at the
 * file's first byte.
 *   lengths  the bytes from start up to the first C-locale white space (TxIds::space) or the window's end;
 *   places   an exclusive sum of length + 1 (+ 0 for an id that does not end in the window) by mgGroupSumKernel (mg_prefix.h);
 *   gather   the bytes and the 0 terminators into one compact buffer.
 * Shape: SIXTEEN LANES an entry, four entries a wave.  Ids are a few to a few tens of bytes (a read name), rarely hundreds, and a window
 * of short reads holds 4e5 of them, 300 bytes apart.  A lane per entry walking bytes makes every load instruction of a wave touch 64
 * different cache lines for 64 bytes wanted and runs as many dependent loads as the id is long; a wave per entry takes one line a step but
 * leaves three quarters of its lanes idle on the common id and needs 4e5 waves.  Sixteen lanes read 16 consecutive bytes a step (one
 * line, seldom two), find the end with the group's 16 bits of one ballot, finish the common id in one to three steps, and in the gather
 * write 16 consecutive bytes a step.  A 10 000-byte id costs its group 625 steps: rare, and it holds back one wave.
 * No lane reads at or beyond byte n of the window: a position there counts as the end.  Only a window's last entry can be left open (an id
 * ends before the next header starts); the gather kernel says so, and whether its header is the next window's first byte, in place[cnt]. */
#define TX_ID_LANES 16
#define TX_ID_THREADS 256
__device__ __forceinline__ bool txSpace (U32 c) { return c == ' ' || (c >= 9 && c <= 13); }      /* TxIds::space */
/* where entry g's id starts in the window: n or more = no byte of it is here */
__device__ __forceinline__ U64 txIdStart (U32 g, U32 nPre, U64 preStart, const U64 *__restrict__ src, U64 add, U64 off)
{ return g < nPre ? preStart : src[g - nPre] + add - off; }

__global__ __launch_bounds__ (TX_ID_THREADS)
void mgTextIdLenKernel (const unsigned char *__restrict__ text, U64 n, const U64 *__restrict__ src, U64 add, U64 off, U32 nPre, U64 preStart, U32 cnt,
                        U32 *__restrict__ len, U32 *__restrict__ lenT)
{
  const U32 g = (blockIdx.x * TX_ID_THREADS + threadIdx.x) / TX_ID_LANES, l = threadIdx.x & (TX_ID_LANES - 1);
  const U32 shift = (threadIdx.x & 63u) & ~(U32) (TX_ID_LANES - 1);      /* the group's bits in the wave's ballot */
  const bool live = g < cnt;
  const U64 start = live ? txIdStart (g, nPre, preStart, src, add, off) : n;
  U64 p = start, end = start;
  bool done = start >= n;                                  /* (uniform over the group, as everything below but q and sp) */
  for (;;)
    { bool sp = false;
      if (!done) { const U64 q = p + l; sp = q >= n || txSpace (text[q]); }
      const U64 b = __ballot (sp);
      if (!done)
        { const U32 m = (U32) (b >> shift) & 0xffffu;
          if (m) { end = p + (U64) (__ffs (m) - 1); done = true; }
          else p += TX_ID_LANES;
        }
      if (!__any (!done)) break;
    }
  if (live && l == 0)
    { const U32 L = (U32) (end - start);                   /* end <= n where start < n; end == start otherwise */
      len[g] = L; lenT[g] = L + (end < n ? 1u : 0u);
    }
}

__global__ __launch_bounds__ (TX_ID_THREADS)
void mgTextIdGatherKernel (const unsigned char *__restrict__ text, U64 n, const U64 *__restrict__ src, U64 add, U64 off, U32 nPre, U64 preStart, U32 cnt,
                           const U32 *__restrict__ len, const U32 *__restrict__ lenT, U32 *place, unsigned char *__restrict__ out)
{
  const U32 g = (blockIdx.x * TX_ID_THREADS + threadIdx.x) / TX_ID_LANES, l = threadIdx.x & (TX_ID_LANES - 1);
  if (g >= cnt) return;
  const U64 start = txIdStart (g, nPre, preStart, src, add, off);
  const U32 L = len[g], o = place[g];
  const bool closed = lenT[g] > L;
  for (U32 i = l ; i < L ; i += TX_ID_LANES) out[o + i] = text[start + i];      /* start + L <= n */
  if (l == 0 && closed) out[o + L] = 0;
  if (l == 0 && g == cnt - 1) place[cnt] = (closed ? 1u : 0u) | (start > n ? 2u : 0u);      /* the last entry: it ended here; its header is the next window's first byte */
}

/* the ids of a window through the kernels, appended to ids as TxIds::headers does from the page-locked window: dSrc[0 .. nSrc) + add - off are
   the id starts in the window (dText, n bytes, the text's byte off first), headerAt0: a header at the window's byte 0 that dSrc does not
   list (the FASTQ file's first).  The stream is waited for.  0 / -1 */
static int txIdsDevice (TxBufs &t, TxIds &ids, const unsigned char *dText, size_t n, const U64 *dSrc, U64 add, U64 off, size_t nSrc, bool headerAt0, hipStream_t st)
{
  const char *what = "record ids on the device";
  const bool cont = ids.open;                              /* the first entry continues the id the window before left open: no new id */
  const U32 nPre = cont || headerAt0 ? 1u : 0u;
  const U64 preStart = cont ? (ids.skipOne ? 1 : 0) : 1;
  const size_t cnt = nSrc + nPre;
  if (!cnt) return 0;
  if ((U64) n + cnt >= 0xffffffffull) { mgSetError ("device text parser: a window of %zu bytes is too large for the id kernels", n); return -1; }
  const double tA = mgNowS ();
  if (t.dIdLen.reserve (cnt, cnt + cnt / 4 + 64, what) || t.dIdLenT.reserve (cnt, cnt + cnt / 4 + 64, what) || t.dIdPlace.reserve (cnt + 2, cnt + cnt / 4 + 66, what)) return -1;
  const unsigned grid = (unsigned) ((cnt * TX_ID_LANES + TX_ID_THREADS - 1) / TX_ID_THREADS);
  U32 *hTotal = (U32 *) (t.hCounts + 6);                   /* page-locked: the scan's total lands where the host reads it */
  hipLaunchKernelGGL (mgTextIdLenKernel, dim3 (grid), dim3 (TX_ID_THREADS), 0, st, dText, (U64) n, dSrc, add, off, nPre, preStart, (U32) cnt, t.dIdLen.p, t.dIdLenT.p);
  hipLaunchKernelGGL ((mgGroupSumKernel<U32, U32>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, t.dIdLenT.p, t.dIdPlace.p, (U32) cnt, hTotal);
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (st) != hipSuccess) return mgHipFail (hipGetLastError (), what), -1;
  const size_t total = *hTotal, bytesCap = (total + 8) & ~(size_t) 7, placeBytes = ((cnt + 1) * 4 + 7) & ~(size_t) 7;
  if (t.dIdBytes.reserve (bytesCap, bytesCap + bytesCap / 4, what)) return -1;
  if (!t.hIdBytes.reserve (bytesCap) || !t.hIdPlace.reserve (placeBytes / 4)) { mgSetError ("record ids on the device: no page-locked memory"); return -1; }
  hipLaunchKernelGGL (mgTextIdGatherKernel, dim3 (grid), dim3 (TX_ID_THREADS), 0, st, dText, (U64) n, dSrc, add, off, nPre, preStart, (U32) cnt,
                      t.dIdLen.p, t.dIdLenT.p, t.dIdPlace.p, t.dIdBytes.p);
  if (hipGetLastError () != hipSuccess) return mgHipFail (hipGetLastError (), what), -1;
  /* both land in page-locked memory by a kernel's stores, not by the copy engine, which is busy with the next window (mgCopyOutPinned) */
  if (mgCopyOutPinned (t.hIdBytes.p, t.dIdBytes.p, bytesCap, (void *) st) != MG_OK || mgCopyOutPinned (t.hIdPlace.p, t.dIdPlace.p, placeBytes, (void *) st) != MG_OK) return -1;
  const size_t base = ids.bytes.size (), skip = cont ? 1 : 0;
  ids.bytes.insert (ids.bytes.end (), (const char *) t.hIdBytes.p, (const char *) t.hIdBytes.p + total);
  size_t at = ids.off.size ();
  ids.off.resize (at + cnt - skip);
  for (size_t i = skip ; i < cnt ; ++i) ids.off[at++] = (U64) base + t.hIdPlace.p[i];
  const U32 flags = t.hIdPlace.p[cnt];
  ids.open = !(flags & 1u); ids.skipOne = (flags & 2u) != 0;
  ids.tDev += mgNowS () - tA;
  return 0;
}

/* ---- the ids of this window (mg_text_int.h) ---- */
/* The positions go out by a kernel's stores (mgCopyOutPinned, which waits for the stream): a copy from the device took its turn behind the NEXT window's
   128 MiB on its way to the device, 2 ms a window, as long as extracting the ids */
int txHeadersOut (TxBufs &t, bool toHost, const TxHdrs &h, hipStream_t st)
{
  if (!toHost || !h.n) return hipStreamSynchronize (st) == hipSuccess ? 0 : -1;
  return t.hHdr.reserve (h.n) && mgCopyOutPinned (t.hHdr.p, h.dSrc, h.n * 8, (void *) st) == MG_OK ? 0 : -1;
}
int txWindowIds (TxBufs &t, TxIds &ids, bool devIds, const TxWalk &wk, const TxHdrs &h, int nThreads, hipStream_t st)
{
  if (devIds) return txIdsDevice (t, ids, wk.dText (), wk.got.n, h.dSrc, h.add, wk.off, h.n, h.at0, st);
  const unsigned char *win = wk.hText ();                  /* while the text is in the page-locked buffer */
  if (ids.open) ids.feed (win, wk.got.n);
  ids.hdr.assign (t.hHdr.p, t.hHdr.p + h.n);
  for (auto &p : ids.hdr) p = p + h.add - 1 - wk.off;      /* the header's first byte in this window (or the window's end: the next window's first byte) */
  if (h.at0) ids.hdr.insert (ids.hdr.begin (), (U64) 0);
  ids.headers (win, wk.got.n, ids.hdr, nThreads);
  return 0;
}
