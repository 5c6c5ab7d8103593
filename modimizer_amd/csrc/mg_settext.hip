/* mg_settext.hip — modutils -rt (modutils.c:169-190) on the device: the lines of a set's text table parsed where the set is built.
 *
 * The host (mgModsetReadText, mg_modsettext.c) reads the header line, makes the set and hands over the rest of the file.  It comes here
 * as it is: parallel pread into one of two page-locked buffers (the file mover of mg_textwin.hip), one copy across the link, and per
 * window of text
 *
 *   lines   newlines counted per tile of 4 KiB, the counts scanned, the newline positions written in order (the same kernel twice);
 *   parse   one lane per line against the strict grammar -- what -wt writes: "-?[0-9]{1,9}" TAB, a token of 1..32 bytes without white
 *           space, TAB, "[0-9]{1,9}" TAB, "[0-9]{1,9}" "\n" -- giving key[], depth[] (the int truncated to 16 bits), info[] (to 8)
 *           and ONE flag for the file: some line is not of that form, or its token is not k bytes long;
 *   carry   the bytes after the window's last newline moved in front of the other window buffer, where the next window continues them.
 *
 * Everything a window's kernels need from the one before (lines done, bytes carried, the flag) is in a small state block on the
 * device, so the host enqueues window after window without waiting and reads the state once, at the end of the file.  A line that does
 * not fit the carry area (128 bytes; a line of the grammar has at most 66) raises the flag.  A file that raises it is parsed again on
 * the host by the reference's own fscanf format (mg_modsettext.c): the device takes the regular file, the host the irregular one.
 *
 * Then the set: modsetAddBatchDevice gives every line its index in order of first occurrence, as modsetIndexFind (.., true) line after
 * line does; the reference assigns depth[index] and info[index] on every line, so the LAST line of a k-mer wins: an atomicMax of the
 * line ordinal per index, and a second pass in which the line whose ordinal won writes its two values.
 */
#include <string.h>
#include <fcntl.h>
#include <unistd.h>
#include <sys/stat.h>
#include "mg_prefix.h"
#include "mg_internal.h"

static bool stTiming (void) { return mgKnobs ()->textTiming == 1; }      /* dev knob (MODGPU_TEXT_TIMING, as the FASTA parser's): the phases to stderr */

#define ST_THREADS 256
#define ST_PER     16                                    /* bytes per lane: one 16-byte load */
#define ST_TILE    (ST_THREADS * ST_PER)                 /* 4 KiB of text per workgroup */
#define ST_CARRY   128u                                  /* bytes kept in front of a window for the line the window before left open */
#define ST_SCAN_THREADS MG_GROUP_THREADS
#define ST_MIN_LINE 8u                                   /* "1\ta\t1\t1\n": a window of n bytes holds at most n / 8 lines of the grammar */

struct StState {                                         /* device resident, carried from window to window */
  U64 linesDone, want;
  U32 carry;                                             /* bytes of an open line in front of the window to come */
  U32 bad;                                               /* a line that is not of the grammar, or wanted lines that are not there */
  U32 nLines;                                            /* lines of the current window that are parsed */
  U32 lastEnd;                                           /* one past the current window's last newline (0: it has none) */
};

/* the newlines of [ST_CARRY - carry, nBytes) of the window buffer.  EMIT false: their number per tile and one past the tile's last;
   EMIT true: their positions, in order, at nl[tileOff[tile] ...] (those that have room) */
template <bool EMIT>
__global__ __launch_bounds__ (ST_THREADS) void mgSetTextLinesKernel (const unsigned char *__restrict__ text, U32 nBytes, const StState *__restrict__ st,
                                                                     U32 *__restrict__ tileCount, U32 *__restrict__ tileLast,
                                                                     const U32 *__restrict__ tileOff, U32 *__restrict__ nl, U32 nlCap)
{
  __shared__ U32 lds[ST_THREADS / 64];
  const U32 start = ST_CARRY - st->carry;
  const U32 base = blockIdx.x * ST_TILE + threadIdx.x * ST_PER;            /* (the buffer is padded to whole tiles) */
  const uint4 v = *(const uint4 *) (text + base);
  const U32 w[4] = { v.x, v.y, v.z, v.w };
  U32 m = 0;
  #pragma unroll
  for (int b = 0 ; b < ST_PER ; ++b)
    { const U32 c = (w[b >> 2] >> (8 * (b & 3))) & 0xffu, pos = base + (U32) b;
      if (c == '\n' && pos >= start && pos < nBytes) m |= 1u << b;
    }
  const U32 cnt = (U32) __popc (m);
  U32 tot;
  const U32 inc = mgBlockInclusive<ST_THREADS, MgSum> (cnt, lds, &tot);
  if (!EMIT)
    { const U32 last = mgBlockReduce<ST_THREADS, MgMax> (m ? base + (32u - (U32) __clz ((int) m)) : 0u, lds);      /* one past the tile's last newline */
      if (threadIdx.x == 0) { tileCount[blockIdx.x] = tot; tileLast[blockIdx.x] = last; }
    }
  else
    { U32 at = tileOff[blockIdx.x] + inc - cnt;
      while (m)
        { const U32 b = (U32) __ffs ((int) m) - 1u; m &= m - 1u;
          if (at < nlCap) nl[at] = base + b;
          ++at;
        }
    }
}

/* one workgroup: tileOff[] = exclusive sum of tileCount[], the window's last newline, and how many of its lines are parsed */
__global__ __launch_bounds__ (ST_SCAN_THREADS) void mgSetTextScanKernel (const U32 *__restrict__ tileCount, const U32 *__restrict__ tileLast, U32 nTiles,
                                                                         U32 *__restrict__ tileOff, U32 nlCap, StState *__restrict__ st)
{
  __shared__ U32 lds[ST_SCAN_THREADS];
  const U32 lines = mgGroupScan<MgSum> (tileCount, tileOff, nTiles, 0u, lds);
  U32 mx = 0;
  for (U32 i = threadIdx.x ; i < nTiles ; i += ST_SCAN_THREADS) { const U32 l = tileLast[i]; mx = l > mx ? l : mx; }
  const U32 last = mgBlockReduce<ST_SCAN_THREADS, MgMax> (mx, lds);
  if (threadIdx.x == 0)
    { const U64 left = st->want - st->linesDone;
      U32 n = (U64) lines < left ? lines : (U32) left;
      if (n > nlCap) { n = nlCap; st->bad = 1; }         /* more lines than lines of the grammar fit: some line is shorter than any of them */
      st->nLines = n; st->lastEnd = last;
    }
}

__device__ __forceinline__ bool stIsSpace (U32 c) { return c == ' ' || (c >= 9u && c <= 13u); }
__device__ __forceinline__ bool stIsDigit (U32 c) { return c - '0' < 10u; }
/* 1..9 digits at text[p ..): the value; p moves past them; false if there are none or more */
__device__ __forceinline__ bool stNumber (const unsigned char *__restrict__ text, U32 &p, U32 e, U32 *val)
{
  U32 x = 0, n = 0;
  while (p < e && stIsDigit (text[p]) && n < 10u) { x = x * 10u + (text[p] - '0'); ++p; ++n; }
  *val = x;
  return n >= 1u && n <= 9u;
}

/* line r of the window, one lane each: from one past the newline before it (the window's first line: from where the carried bytes
   start) to its own newline */
__global__ __launch_bounds__ (256) void mgSetTextParseKernel (const unsigned char *__restrict__ text, const U32 *__restrict__ nl, StState *__restrict__ st,
                                                              int k, U64 *__restrict__ key, U16 *__restrict__ depth, U8 *__restrict__ info)
{
  const U32 n = st->nLines;
  const U64 g0 = st->linesDone;
  for (U32 r = blockIdx.x * blockDim.x + threadIdx.x ; r < n ; r += gridDim.x * blockDim.x)
    { U32 p = r ? nl[r - 1] + 1u : ST_CARRY - st->carry;
      const U32 e = nl[r];
      bool ok = true;
      U32 ignore, d = 0, f = 0, tlen = 0;
      U64 x = 0;
      if (p < e && text[p] == '-') ++p;
      ok = stNumber (text, p, e, &ignore) && p < e && text[p] == '\t';
      if (ok)
        { ++p;
          while (p < e && tlen <= 32u)
            { const U32 c = text[p];
              if (stIsSpace (c) || !c) break;                                  /* (a 0 byte ends the reference's loop over the token: such a line is the host parser's) */
              const U32 l = c | 0x20u;
              x = (x << 2) | (U64) (l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 0u);      /* modutils.c:178-184 */
              ++tlen; ++p;
            }
          ok = tlen >= 1u && tlen <= 32u && p < e && text[p] == '\t';
        }
      if (ok) { ++p; ok = stNumber (text, p, e, &d) && p < e && text[p] == '\t'; }
      if (ok) { ++p; ok = stNumber (text, p, e, &f) && p == e; }
      if (!ok || tlen != (U32) k) st->bad = 1;
      key[g0 + r] = x; depth[g0 + r] = (U16) d; info[g0 + r] = (U8) f;
    }
}

/* one wave, after the window's parse: the bytes behind its last newline go in front of the other window buffer */
__global__ __launch_bounds__ (64) void mgSetTextCarryKernel (const unsigned char *__restrict__ text, U32 nBytes, unsigned char *__restrict__ other, StState *__restrict__ st)
{
  const U32 start = ST_CARRY - st->carry;
  const U32 from = st->lastEnd ? st->lastEnd : start;
  const U32 len = nBytes - from;
  const U64 done = st->linesDone + st->nLines;
  const bool open = done < st->want;                     /* what follows the last wanted line is not looked at */
  const bool fits = len <= ST_CARRY;
  if (open && fits) for (U32 i = threadIdx.x ; i < len ; i += 64u) other[ST_CARRY - len + i] = text[from + i];
  __syncthreads ();
  if (threadIdx.x == 0)
    { st->linesDone = done;
      st->carry = open && fits ? len : 0u;
      if (open && !fits) st->bad = 1;
    }
}

/* last line wins: win[index] = the highest 1-based ordinal of the lines with that index; then the line that won writes */
__global__ void mgSetTextLastKernel (const U32 *__restrict__ idx, U64 n, U32 *__restrict__ win)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x) atomicMax (&win[idx[i]], (U32) (i + 1));
}
__global__ void mgSetTextPlaceKernel (const U32 *__restrict__ idx, U64 n, const U32 *__restrict__ win, const U16 *__restrict__ depth, const U8 *__restrict__ info,
                                      U16 *__restrict__ outDepth, U8 *__restrict__ outInfo)
{
  for (U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x ; i < n ; i += (U64) gridDim.x * blockDim.x)
    { const U32 ix = idx[i];
      if (win[ix] == (U32) (i + 1)) { outDepth[ix] = depth[i]; outInfo[ix] = info[i]; }
    }
}

/* ---------------------------------------------------------------------------------------- */
/* host side                                                                                  */

struct StBufs {                                          /* of one call: its device arrays are the scratch's, the three that hold the result named here */
  MgDevScratch scratch { "set text parse on the device" };
  U64 *dKey = 0; U16 *dDepth = 0; U8 *dInfo = 0;
  unsigned char *hPin[2] = { 0, 0 };
  hipEvent_t copied[2]; bool ev[2] = { false, false };
  StState *hState = 0;
  int fd = -1;
  ~StBufs ()
  { for (int i = 0 ; i < 2 ; ++i) { if (hPin[i]) (void) hipHostFree (hPin[i]); if (ev[i]) (void) hipEventDestroy (copied[i]); }
    if (hState) (void) hipHostFree (hState);
    if (fd >= 0) close (fd);
  }
};

static MgStatus stParse (StBufs &b, const char *filename, U64 bodyOff, U64 want, int k, int *verdict)
{
  MgStatus s = mgEnsureDevice (); if (s) return s;
  b.fd = open (filename, O_RDONLY);
  struct stat sb;
  if (b.fd < 0 || fstat (b.fd, &sb)) { mgSetError ("failed to open text file %s", filename); return MG_ERR_ARG; }
  const U64 fileSize = (U64) sb.st_size;
  const U64 body = fileSize > bodyOff ? fileSize - bodyOff : 0;
  if (body < want * ST_MIN_LINE) { *verdict = 1; return MG_OK; }          /* (fewer bytes than that many lines take: the host parser names the line) */
  /* windows of at most 32 MiB: the text is parsed as fast as it is read, and two page-locked buffers are made per call */
  const size_t window = mgTextWindowBytes ((size_t) (body < ((U64) 32 << 20) ? body : ((U64) 32 << 20)));
  const U32 nlCap = (U32) ((window + ST_CARRY) / ST_MIN_LINE + 2);
  const size_t bufBytes = ST_CARRY + window + ST_TILE;
  const U32 maxTiles = (U32) (bufBytes / ST_TILE + 1);
  hipStream_t st = 0;
  const double t0 = mgNowS (); double tRead = 0, tWait = 0;
  unsigned char *dText[2]; StState *dState; U32 *dTileCount, *dTileLast, *dTileOff, *dNl;
  for (int i = 0 ; i < 2 ; ++i)
    { MG_HIP (hipHostMalloc ((void **) &b.hPin[i], window, hipHostMallocDefault));
      if (b.scratch.get (&dText[i], bufBytes)) return MG_ERR_HIP;
      MG_HIP (hipEventCreateWithFlags (&b.copied[i], hipEventDisableTiming)); b.ev[i] = true;
    }
  if (b.scratch.get (&dState, 1)) return MG_ERR_HIP;
  MG_HIP (hipHostMalloc ((void **) &b.hState, sizeof (StState), hipHostMallocDefault));
  if (b.scratch.get (&dTileCount, maxTiles) || b.scratch.get (&dTileLast, maxTiles) || b.scratch.get (&dTileOff, maxTiles) || b.scratch.get (&dNl, nlCap)
      || b.scratch.get (&b.dKey, want) || b.scratch.get (&b.dDepth, want) || b.scratch.get (&b.dInfo, want)) return MG_ERR_HIP;
  StState init; memset (&init, 0, sizeof (init)); init.want = want;
  MG_HIP (hipMemcpyAsync (dState, &init, sizeof (init), hipMemcpyHostToDevice, st));
  MG_HIP (hipStreamSynchronize (st));                    /* (init is on this stack) */
  const double t1 = mgNowS ();
  int w = 0;
  for (U64 off = 0 ; off < body ; ++w)
    { const int cur = w & 1;
      const size_t nCur = body - off < window ? (size_t) (body - off) : window;
      const double r0 = mgNowS ();
      if (w >= 2) MG_HIP (hipEventSynchronize (b.copied[cur]));            /* the buffer's last copy to the device is over */
      const double r1 = mgNowS ();
      if (mgTextReadParallel (b.fd, b.hPin[cur], nCur, (int64_t) (bodyOff + off))) { mgSetError ("failed to read text file %s", filename); return MG_ERR_ARG; }
      tWait += r1 - r0; tRead += mgNowS () - r1;
      MG_HIP (hipMemcpyAsync (dText[cur] + ST_CARRY, b.hPin[cur], nCur, hipMemcpyHostToDevice, st));
      MG_HIP (hipEventRecord (b.copied[cur], st));
      const U32 nBytes = ST_CARRY + (U32) nCur, nTiles = (nBytes + ST_TILE - 1) / ST_TILE;
      MG_LAUNCH (MG_K_SETTEXT_LINES, st, mgSetTextLinesKernel<false>, dim3 (nTiles), dim3 (ST_THREADS), 0, st, dText[cur], nBytes, dState,
                 dTileCount, dTileLast, dTileOff, dNl, nlCap);
      MG_LAUNCH (MG_K_SETTEXT_SCAN, st, mgSetTextScanKernel, dim3 (1), dim3 (ST_SCAN_THREADS), 0, st, dTileCount, dTileLast, nTiles, dTileOff, nlCap, dState);
      MG_LAUNCH (MG_K_SETTEXT_LINES, st, mgSetTextLinesKernel<true>, dim3 (nTiles), dim3 (ST_THREADS), 0, st, dText[cur], nBytes, dState,
                 dTileCount, dTileLast, dTileOff, dNl, nlCap);
      MG_LAUNCH (MG_K_SETTEXT_PARSE, st, mgSetTextParseKernel, dim3 (mgGrid (nlCap)), dim3 (256), 0, st, dText[cur], dNl, dState, k, b.dKey, b.dDepth, b.dInfo);
      MG_LAUNCH (MG_K_SETTEXT_SCAN, st, mgSetTextCarryKernel, dim3 (1), dim3 (64), 0, st, dText[cur], nBytes, dText[cur ^ 1], dState);
      MG_HIP (hipMemcpyAsync (b.hState, dState, sizeof (StState), hipMemcpyDeviceToHost, st));
      MG_HIP (hipGetLastError ());
      off += nCur;
      /* (a look at the state as the window before last left it, without waiting: nothing after the last wanted line is read) */
      if (w >= 2 && ((volatile StState *) b.hState)->linesDone >= want) break;
      if (w >= 2 && ((volatile StState *) b.hState)->bad) break;
    }
  const double t2 = mgNowS ();
  MG_HIP (hipStreamSynchronize (st));
  MG_HIP (hipMemcpy (b.hState, dState, sizeof (StState), hipMemcpyDeviceToHost));
  if (stTiming ())
    fprintf (stderr, "  [set text] parse: %d windows of %zu bytes; buffers %.3f s, file read %.3f, waits for a window's copy %.3f, enqueue + rest %.3f, wait at the end %.3f\n",
             w, window, t1 - t0, tRead, tWait, t2 - t1 - tRead - tWait, mgNowS () - t2);
  *verdict = (b.hState->bad || b.hState->linesDone < want) ? 1 : 0;
  return MG_OK;
}

extern "C" int mgSetTextParseDevice (const char *filename, U64 bodyOff, U64 want, int k, U64 **dKey, U16 **dDepth, U8 **dInfo)
{
  *dKey = 0; *dDepth = 0; *dInfo = 0;
  if (!want) return 0;
  StBufs b;
  int verdict = 1;
  if (stParse (b, filename, bodyOff, want, k, &verdict)) return -1;
  if (verdict) return 1;
  *dKey = b.scratch.take (b.dKey); *dDepth = b.scratch.take (b.dDepth); *dInfo = b.scratch.take (b.dInfo);      /* the caller's from here */
  return 0;
}

static MgStatus stFill (Modset *ms, const U64 *dKey, const U16 *dDepth, const U8 *dInfo, U64 n)
{
  MgStatus s = mgEnsureDevice (); if (s) return s;
  if (!n) return MG_OK;
  hipStream_t st = 0;
  MgDevScratch scratch ("set text fill on the device");
  U32 *dIdx, *dWin; U16 *dOutDepth; U8 *dOutInfo;
  const double t0 = mgNowS ();
  if (scratch.get (&dIdx, n)) return MG_ERR_HIP;
  const U64 piece = (U64) 1 << 30;                       /* modsetAddBatchDevice takes fewer than 2^31 a call */
  for (U64 off = 0 ; off < n ; off += piece)
    if ((s = modsetAddBatchDevice (ms, dKey + off, n - off < piece ? n - off : piece, dIdx + off, 0, (void *) st))) return s;
  MG_HIP (hipStreamSynchronize (st));
  const double t1 = mgNowS ();
  const size_t m1 = (size_t) ms->max + 1;
  if (scratch.get (&dWin, m1) || scratch.get (&dOutDepth, m1) || scratch.get (&dOutInfo, m1)) return MG_ERR_HIP;
  MG_HIP (hipMemsetAsync (dWin, 0, m1 * 4, st)); MG_HIP (hipMemsetAsync (dOutDepth, 0, m1 * 2, st)); MG_HIP (hipMemsetAsync (dOutInfo, 0, m1, st));
  MG_LAUNCH (MG_K_SETTEXT_LAST, st, mgSetTextLastKernel, dim3 (mgGrid (n)), dim3 (256), 0, st, dIdx, n, dWin);
  MG_LAUNCH (MG_K_SETTEXT_LAST, st, mgSetTextPlaceKernel, dim3 (mgGrid (n)), dim3 (256), 0, st, dIdx, n, dWin, dDepth, dInfo, dOutDepth, dOutInfo);
  MG_HIP (hipGetLastError ());
  MG_HIP (hipStreamSynchronize (st));
  const double t2 = mgNowS ();
  /* the host's depth[] and info[] are the authority; the device table's depth copy follows them */
  if ((s = mgCopyD2HBig (ms->depth, dOutDepth, m1 * 2)) || (s = mgCopyD2HBig (ms->info, dOutInfo, m1))) return s;
  s = mgModsetAdoptDepthDevice (ms, dOutDepth);
  if (stTiming ())
    fprintf (stderr, "  [set text] fill: insert (device table made) %.3f s, last line wins %.3f, depth[] + info[] to the host %.3f\n", t1 - t0, t2 - t1, mgNowS () - t2);
  return s;
}

extern "C" int mgSetTextFillDevice (Modset *ms, const U64 *dKey, const U16 *dDepth, const U8 *dInfo, U64 n)
{ return stFill (ms, dKey, dDepth, dInfo, n) ? -1 : 0; }

extern "C" int mgSetTextFillHostArrays (Modset *ms, const U64 *key, const U16 *depth, const U8 *info, U64 n)
{
  if (mgEnsureDevice ()) return -1;
  if (!n) return 0;
  MgDevScratch scratch ("mgModsetReadText");
  U64 *dKey; U16 *dDepth; U8 *dInfo;
  if (scratch.get (&dKey, n) || scratch.get (&dDepth, n) || scratch.get (&dInfo, n)) return -1;
  if (mgCopyH2DBig (dKey, key, n * 8) || mgCopyH2DBig (dDepth, depth, n * 2) || mgCopyH2DBig (dInfo, info, n)) return -1;
  return stFill (ms, dKey, dDepth, dInfo, n) ? -1 : 0;
}
