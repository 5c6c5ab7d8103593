/* mg_composition.hip — the reference's `composition` program (composition.c:32-121 over seqIOopenRead (file, 0, true) / seqIOread,
 * seqio.c:30-73,234-346) on the device: how many records, how long, which bases, which qualities, the length bins of -l.
 *
 * The text goes through the device text parser's window loop (mgTextStreamWindows, mg_textwin.hip) and is read by that parser's rules
 * (txLoad / txEvent / txNewlines, mg_internal.h); nothing is written per byte.  Four launches a window:
 *
 *   FASTA   A1  per tile of 4 KiB: the code of its last event (the parser's own K1);
 *           A2  one workgroup: the running maximum over the tiles, on top of the state the window before ended in;
 *           A3  per tile, the work: what every byte is (header / kept / dropped: dna2textAmbigConv, seqio.c:49,322,621-630), the 256-bin
 *               histogram of the kept bytes, and the records that END inside the tile -- a record ends at the next record start, its length
 *               is the kept bytes since its own start.  "Kept bytes so far" is a prefix sum, "kept bytes at the last start" a running
 *               maximum of that (the sum only grows), so a segmented sum is two plain scans: inside the tile here, over the tiles in
 *           A4  one workgroup: the records that start in one tile and end at the first start of a later one (of a later window, too: the
 *               two running values are carried in CpState), and the tiles' lenMin pairs folded in file order.
 *   FASTQ   Q1  per tile: its newlines, the position of its last one, and its non-newline bytes by line number mod 4 relative to the tile;
 *           Q2  one workgroup: the line number at every tile's first byte, the last newline before it, and -- now that the phase of every
 *               tile is known -- the sequence-line bytes minus the quality-line bytes before it;
 *           Q3  per tile, the work: line mod 4 says what a byte is; the two histograms; a record is complete at its fourth newline, its
 *               length is that newline's position less the one before (the quality line's, which IS the sequence's length unless the
 *               running difference is non-zero there: seqio.c:338); '@' and '+' at the line starts (seqio.c:302,333);
 *           Q4  one workgroup: the tiles' lenMin pairs folded in file order.
 *
 * lenMin (composition.c:64: `if (!lenMin || seqLen < lenMin) lenMin = seqLen`) is reset by an empty record, so it is not a minimum.  A run
 * of records acts on it as a pair (e: it holds an empty record, m: the least length after the last empty one, or of all); pairs combine
 * associatively -- (e1, m1) then (e2, m2) = e2 ? (1, m2) : (e1, min (m1, m2)) -- and over a range that is "the last part with e set, and
 * the minimum of m from there on": one maximum and one minimum, which is how threads, tiles and windows are folded.
 *
 * Counters: what a thread or a tile counts is 32-bit and bounded by the tile's 4096 bytes (the LDS histograms: by the bytes of one launch,
 * a window of at most 2^31); everything that adds up across tiles -- CpState, the bins' sums -- is 64-bit.
 *
 * What ends a file early is found on the device as a minimum (of file offsets, of line numbers) and judged on the host, as the FASTQ parser
 * does.  A last record the reference drops as unfinished (seqio.c:215-219) has been counted by then: the host learns where it starts and
 * the text before that point goes through once more -- twice the work, for files that are cut off. */
#include <fcntl.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <vector>
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_textsrc.h"

#define CP_THREADS 256
#define CP_WAVES   (CP_THREADS / 64)
#define CP_TILE    (CP_THREADS * 16)
static_assert (CP_TILE == MG_TEXT_TILE, "the parser's tile");
#define CP_NONE    (~(U64) 0)
#define CP_MAXLEN  ((U64) 1 << 31)                      /* the reference's lengths are int */
#define CP_GRID    2048                                  /* workgroups of the work kernels: each walks tiles grid-stride and flushes its LDS counters once */
/* the shape of the LDS histogram (DESIGN_EXPERIMENTS.md "composition: the histogram"): 0 one histogram a workgroup, one atomic a byte;
   1 one histogram a wave, one atomic a byte; 2 one a wave, a lane adds a run of equal bytes at once */
#ifndef CP_HIST_MODE
#define CP_HIST_MODE 2
#endif
#define CP_HISTS   (CP_HIST_MODE ? CP_WAVES : 1)

struct CpState {                                         /* device resident, carried from window to window; read back once */
  U64 lastEvent;          /* FASTA: code of the text's last event (txEvent): bit 0 = inside a header */
  U64 kept, lastStartK;   /* FASTA: kept bytes so far; kept bytes before the last record start, + 1 (0: no start yet) */
  U64 nl, lastNl, diff;   /* FASTQ: newlines so far; position + 1 of the last one; sequence-line bytes minus quality-line bytes so far */
  U64 newlines;           /* FASTA: newlines so far (the line of "incomplete sequence record") */
  U64 hdrEnd;             /* FASTA: position + 1 of the last newline that ends a header line */
  U64 lastStart;          /* position + 1 of the last record start (FASTA) / of the byte after the last complete record (FASTQ) */
  U64 nSeq, totLen, lenMax, minE, minM;
  U64 errLine;            /* FASTQ: the first line that breaks a rule (line mod 4 says which), CP_NONE */
  U64 badOff, badLine;    /* the first byte the reference indexes a table out of bounds with: file offset, (FASTQ) line; CP_NONE */
  U64 tooLong, binOverflow, crossed, complete;
  U64 base[256], qual[256];
};

__device__ __forceinline__ void cpAdd64 (U64 *p, U64 v) { atomicAdd ((unsigned long long *) p, (unsigned long long) v); }
__device__ __forceinline__ void cpMax64 (U64 *p, U64 v) { atomicMax ((unsigned long long *) p, (unsigned long long) v); }
__device__ __forceinline__ void cpMin64 (U64 *p, U64 v) { atomicMin ((unsigned long long *) p, (unsigned long long) v); }

/* the lenMin pair */
__device__ __forceinline__ void cpMinAdd (U64 &e, U64 &m, U64 len) { if (!len) { e = 1; m = CP_NONE; } else if (len < m) m = len; }
__device__ __forceinline__ void cpMinThen (U64 &e, U64 &m, U64 e2, U64 m2) { if (e2) { e = 1; m = m2; } else if (m2 < m) m = m2; }

/* floor (sqrt (x)) for x < 2^38: composition.c:66's bin `10.*sqrt((double)len)`, truncated, is this of 100 len for every len < 2^31 */
__device__ __forceinline__ U32 cpIsqrt (U64 x)
{
  U64 r = 0;
  for (U64 bit = (U64) 1 << 18 ; bit ; bit >>= 1) { const U64 t = r | bit; if (t * t <= x) r = t; }
  return (U32) r;
}

struct CpAcc { U64 nSeq, totLen, lenMax, minE, minM; };      /* the records a thread finished, in file order */
struct CpBins { U32 *count; U64 *sum; U64 cap; };            /* -l: count == 0 without the flag */

__device__ __forceinline__ void cpRecord (CpAcc &a, U64 len, const CpBins &bins, CpState *st)
{
  ++a.nSeq; a.totLen += len; if (len > a.lenMax) a.lenMax = len;
  cpMinAdd (a.minE, a.minM, len);
  if (len >= CP_MAXLEN) { st->tooLong = 1; return; }
  if (bins.count)
    { const U64 b = cpIsqrt (100 * len);
      if (b < bins.cap) { atomicAdd (&bins.count[b], 1u); cpAdd64 (&bins.sum[b], len); }
      else st->binOverflow = 1;
    }
}

/* a lane's run of equal symbols goes to the histogram at once: a HiFi quality line, a poly-A read are one symbol */
struct CpRun { U32 sym, cnt; };
__device__ __forceinline__ void cpHistAdd (U32 *h, CpRun &r, U32 sym)
{
#if CP_HIST_MODE == 2
  if (sym == r.sym) { ++r.cnt; return; }
  if (r.cnt) atomicAdd (&h[r.sym], r.cnt);
  r.sym = sym; r.cnt = 1;
#else
  atomicAdd (&h[sym], 1u);
#endif
}
__device__ __forceinline__ void cpHistFlush (U32 *h, CpRun &r) { if (r.cnt) atomicAdd (&h[r.sym], r.cnt); r.cnt = 0; }

/* the workgroup's LDS histograms onto the 64-bit ones */
__device__ __forceinline__ void cpHistOut (U32 (*h)[256], U64 *total)
{
  for (U32 i = threadIdx.x ; i < 256 ; i += CP_THREADS)
    { U32 v = 0;
      for (int w = 0 ; w < CP_HISTS ; ++w) v += h[w][i];
      if (v) cpAdd64 (&total[i], v);
    }
}

/* dna2textAmbigConv (seqio.c:621-630): the 15 letters ABCDGHKMNRSTVWY in either case become the upper-case letter, '-' stays, every other
   byte below 0x80 is dropped (0) */
#define CP_AMBIG 0x2dc699eu
__device__ __forceinline__ U32 cpFastaKeep (U32 c)
{
  if (c == '-') return c;
  return ((c & 0xc0u) == 0x40u && ((CP_AMBIG >> (c & 0x1fu)) & 1u)) ? (c & 0xdfu) : 0u;
}

/* the tiles' lenMin pairs, folded in file order onto the state's (one workgroup of MG_GROUP_THREADS; lds: 16 words) */
__device__ __forceinline__ void cpFoldPairs (U64 nTiles, const U32 *tileMinE, const U64 *tileMinM, CpState *st, U64 *lds)
{
  U64 lastE = 0;
  for (U64 t = threadIdx.x ; t < nTiles ; t += MG_GROUP_THREADS) if (tileMinE[t]) lastE = t + 1;
  lastE = mgBlockReduce<MG_GROUP_THREADS, MgMax> (lastE, lds);
  U64 m = CP_NONE;
  for (U64 t = threadIdx.x ; t < nTiles ; t += MG_GROUP_THREADS) if (t + 1 >= lastE && tileMinM[t] < m) m = tileMinM[t];
  m = ~mgBlockReduce<MG_GROUP_THREADS, MgMax> (~m, lds);
  if (threadIdx.x == 0) { U64 e = st->minE, mm = st->minM; cpMinThen (e, mm, lastE ? 1 : 0, m); st->minE = e; st->minM = mm; }
}

/* what a work kernel's threads share across the tiles the workgroup walks */
enum { CP_S_NSEQ = 0, CP_S_TOTLEN, CP_S_LENMAX, CP_S_NEWLINES, CP_S_LASTSTART, CP_S_HDREND, CP_S_COUNT };

/* a thread's finished records into the workgroup's counters, and the tile's pair */
__device__ __forceinline__ void cpTileOut (const CpAcc &a, U64 *sAcc, U32 *s32, U64 *s64, U64 tile, U32 *tileMinE, U64 *tileMinM)
{
  if (a.nSeq) { cpAdd64 (&sAcc[CP_S_NSEQ], a.nSeq); cpAdd64 (&sAcc[CP_S_TOTLEN], a.totLen); cpMax64 (&sAcc[CP_S_LENMAX], a.lenMax); }
  const U32 lastE = mgBlockReduce<CP_THREADS, MgMax> (a.minE ? threadIdx.x + 1u : 0u, s32);
  const U64 inv = mgBlockReduce<CP_THREADS, MgMax> (threadIdx.x + 1u >= lastE ? ~a.minM : (U64) 0, s64);
  if (threadIdx.x == 0) { tileMinE[tile] = lastE ? 1u : 0u; tileMinM[tile] = ~inv; }
}
__device__ __forceinline__ void cpAccOut (U64 *sAcc, CpState *st)
{
  if (threadIdx.x) return;
  if (sAcc[CP_S_NSEQ]) { cpAdd64 (&st->nSeq, sAcc[CP_S_NSEQ]); cpAdd64 (&st->totLen, sAcc[CP_S_TOTLEN]); cpMax64 (&st->lenMax, sAcc[CP_S_LENMAX]); }
  if (sAcc[CP_S_NEWLINES]) cpAdd64 (&st->newlines, sAcc[CP_S_NEWLINES]);
  if (sAcc[CP_S_LASTSTART]) cpMax64 (&st->lastStart, sAcc[CP_S_LASTSTART]);
  if (sAcc[CP_S_HDREND]) cpMax64 (&st->hdrEnd, sAcc[CP_S_HDREND]);
}

/* ======================================================================================== */
/* FASTA                                                                                      */

/* A2: the state at every tile's first byte */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgCompStateScanKernel (U64 *tileEvent, U64 nTiles, CpState *st)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U64 total = mgGroupScan<MgMax> (tileEvent, tileEvent, nTiles, st->lastEvent, lds);
  if (threadIdx.x == 0) st->lastEvent = total;
}

/* A3 */
__global__ __launch_bounds__ (CP_THREADS)
void mgCompFastaKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 prevByte, U64 nTiles, const U64 *__restrict__ tileIn,
                        U32 *__restrict__ tileKept, U32 *__restrict__ tileLastCode, U32 *__restrict__ tileFirstKept, U32 *__restrict__ tileMinE, U64 *__restrict__ tileMinM,
                        int flags, CpBins bins, CpState *st)
{
  __shared__ U32 sHist[CP_HISTS][256];
  __shared__ U64 sAcc[CP_S_COUNT];
  __shared__ U64 s64[CP_WAVES];
  __shared__ U32 s32[CP_WAVES];
  for (U32 i = threadIdx.x ; i < CP_HISTS * 256 ; i += CP_THREADS) (&sHist[0][0])[i] = 0;
  if (threadIdx.x < CP_S_COUNT) sAcc[threadIdx.x] = 0;
  __syncthreads ();
  U32 *hist = sHist[CP_HIST_MODE ? threadIdx.x >> 6 : 0];
  for (U64 tile = blockIdx.x ; tile < nTiles ; tile += gridDim.x)
    { const U64 at = (tile * CP_THREADS + threadIdx.x) * 16;
      unsigned char b[16]; U32 prev0 = 0;
      U64 last = 0;
      if (at < n) { txLoad (text, n, at, prevByte, b, &prev0); last = txLastEvent (b, at, n, prev0, textBase + at); }
      const U64 excl = mgBlockExclusive<CP_THREADS, MgMax> (last, s64);
      const U64 in = excl > tileIn[tile] ? excl : tileIn[tile];
      /* the thread's kept bytes and starts: its place in the tile's two scans */
      U32 k = 0, ns = 0, kAtLast = 0;
      if (at < n)
        { bool header = (in & 1) != 0;
          U32 prev = prev0;
#pragma unroll
          for (int j = 0 ; j < 16 ; ++j)
            { if (at + j < n)
                { const U32 c = b[j];
                  if (c == '>' && prev == '\n') { header = true; ++ns; kAtLast = k; }
                  else if (c == '\n') header = false;
                  else if (!header && cpFastaKeep (c)) ++k;
                }
              prev = b[j];
            }
        }
      U32 tileK;
      const U32 kMine = mgBlockInclusive<CP_THREADS, MgSum> (k, s32, &tileK) - k;      /* kept bytes of the tile before this thread's */
      const U32 code = ns ? kMine + kAtLast + 1 : 0;                                       /* kept bytes of the tile before the thread's last start, + 1 */
      const U32 prevCode = mgBlockExclusive<CP_THREADS, MgMax> (code, s32);
      const U32 lastCode = mgBlockReduce<CP_THREADS, MgMax> (code, s32);
      /* the walk that counts */
      CpAcc a = { 0, 0, 0, 0, CP_NONE };
      U32 nlc = 0;
      if (at < n)
        { bool header = (in & 1) != 0, saw = prevCode != 0;
          U32 prev = prev0, run = saw ? kMine - (prevCode - 1) : kMine;       /* kept bytes since the last start of the tile, or since its first byte */
          U64 bad = CP_NONE, lastStart = 0, hdrEnd = 0;
          CpRun hr = { 0, 0 };
#pragma unroll
          for (int j = 0 ; j < 16 ; ++j)
            { if (at + j < n)
                { const U32 c = b[j];
                  if (c == '>' && prev == '\n')
                    { if (saw) cpRecord (a, run, bins, st);
                      else tileFirstKept[tile] = run;              /* the tile's first start ends a record of an earlier tile: A4 */
                      saw = true; run = 0; header = true; lastStart = textBase + at + j + 1;
                    }
                  else if (c == '\n') { if (header) hdrEnd = textBase + at + j + 1; header = false; ++nlc; }
                  else if (!header)
                    { if (c >= 0x80u) { if (bad == CP_NONE) bad = textBase + at + j; }      /* convert[] has 128 entries (seqio.c:322) */
                      else { const U32 u = cpFastaKeep (c); if (u) { ++run; if (flags & MG_COMP_BASES) cpHistAdd (hist, hr, u); } }
                    }
                }
              prev = b[j];
            }
          cpHistFlush (hist, hr);
          if (bad != CP_NONE) cpMin64 (&st->badOff, bad);
          if (lastStart) cpMax64 (&sAcc[CP_S_LASTSTART], lastStart);
          if (hdrEnd) cpMax64 (&sAcc[CP_S_HDREND], hdrEnd);
        }
      nlc = mgWaveReduce<MgSum> (nlc);
      if ((threadIdx.x & 63u) == 0 && nlc) cpAdd64 (&sAcc[CP_S_NEWLINES], nlc);
      cpTileOut (a, sAcc, s32, s64, tile, tileMinE, tileMinM);
      if (threadIdx.x == 0) { tileKept[tile] = tileK; tileLastCode[tile] = lastCode; }
    }
  __syncthreads ();
  if (flags & MG_COMP_BASES) cpHistOut (sHist, st->base);
  cpAccOut (sAcc, st);
}

/* A4: the records that end at a tile's first start, the pairs in order, the two running values for the next window */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgCompFastaStitchKernel (U64 nTiles, const U32 *__restrict__ tileKept, const U32 *__restrict__ tileLastCode, const U32 *__restrict__ tileFirstKept,
                              U32 *tileMinE, U64 *tileMinM, U64 *tileKoff, U64 *tilePrev, int crossing, CpBins bins, CpState *st)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U64 kTotal = mgGroupScan<MgSum> (tileKept, tileKoff, nTiles, st->kept, lds);
  __syncthreads ();
  for (U64 t = threadIdx.x ; t < nTiles ; t += MG_GROUP_THREADS) tilePrev[t] = tileLastCode[t] ? tileKoff[t] + tileLastCode[t] : 0;
  __syncthreads ();
  const U64 lastStartK = mgGroupScan<MgMax> (tilePrev, tilePrev, nTiles, st->lastStartK, lds);
  __syncthreads ();
  CpAcc a = { 0, 0, 0, 0, CP_NONE };
  for (U64 t = threadIdx.x ; t < nTiles ; t += MG_GROUP_THREADS)
    if (tileLastCode[t] && tilePrev[t])                    /* a start here, and one before it in the text: a record ends */
      { const U64 len = tileKoff[t] + tileFirstKept[t] - (tilePrev[t] - 1);
        CpAcc one = { 0, 0, 0, 0, CP_NONE };
        cpRecord (one, len, bins, st);
        a.nSeq += 1; a.totLen += len; if (len > a.lenMax) a.lenMax = len;
        cpMinThen (one.minE, one.minM, tileMinE[t], tileMinM[t]);      /* that record, then the tile's own */
        tileMinE[t] = (U32) one.minE; tileMinM[t] = one.minM;
      }
  __syncthreads ();
  cpFoldPairs (nTiles, tileMinE, tileMinM, st, lds);
  const U64 nSeq = mgBlockReduce<MG_GROUP_THREADS, MgSum> (a.nSeq, lds), totLen = mgBlockReduce<MG_GROUP_THREADS, MgSum> (a.totLen, lds);
  const U64 lenMax = mgBlockReduce<MG_GROUP_THREADS, MgMax> (a.lenMax, lds);
  if (threadIdx.x == 0)
    { st->nSeq += nSeq; st->totLen += totLen; if (lenMax > st->lenMax) st->lenMax = lenMax;
      st->kept = kTotal; st->lastStartK = lastStartK;
      if (crossing) ++st->crossed;
    }
}

/* the end of the text (its textEnd bytes): the record that is open ends there -- if the reference returns it: the last byte is a newline, and
   not the one that ends a header line (seqio.c:215-219,314-320); force: the text was cut in front of a record start */
__global__ void mgCompFastaFinishKernel (U32 lastByte, U64 textEnd, int force, CpBins bins, CpState *st)
{
  if (threadIdx.x || blockIdx.x) return;
  const bool complete = force || (lastByte == '\n' && st->hdrEnd != textEnd);
  st->complete = complete ? 1 : 0;
  if (!complete || !st->lastStartK) return;
  const U64 len = st->kept - (st->lastStartK - 1);
  CpAcc one = { 0, 0, 0, 0, CP_NONE };
  cpRecord (one, len, bins, st);
  st->nSeq += 1; st->totLen += len; if (len > st->lenMax) st->lenMax = len;
  U64 e = st->minE, m = st->minM; cpMinThen (e, m, one.minE, one.minM); st->minE = e; st->minM = m;
}

/* ======================================================================================== */
/* FASTQ                                                                                      */

/* Q1: per tile its newlines, position + 1 of the last one, and its other bytes by (newlines of the tile before the byte) mod 4, 16 bits each */
__global__ __launch_bounds__ (CP_THREADS)
void mgCompLinesKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 *__restrict__ tileNl, U64 *__restrict__ tileLastNl, U64 *__restrict__ tileCnt)
{
  __shared__ U64 s64[CP_WAVES];
  __shared__ U32 s32[CP_WAVES];
  const U64 at = ((U64) blockIdx.x * CP_THREADS + threadIdx.x) * 16;
  unsigned char b[16]; U32 prev = 0, nl = 0; U64 lastNl = 0;
  if (at < n)
    { txLoad (text, n, at, 0, b, &prev);
      nl = txNewlines (b, at, n);
#pragma unroll
      for (int j = 0 ; j < 16 ; ++j) if (at + j < n && b[j] == '\n') lastNl = textBase + at + j + 1;
    }
  U32 total;
  U32 line = mgBlockInclusive<CP_THREADS, MgSum> (nl, s32, &total) - nl;
  U64 cnt = 0;
  if (at < n)
    {
#pragma unroll
      for (int j = 0 ; j < 16 ; ++j)
        if (at + j < n) { if (b[j] == '\n') ++line; else cnt += (U64) 1 << (16 * (line & 3u)); }
    }
  cnt = mgBlockReduce<CP_THREADS, MgSum> (cnt, s64);           /* each of the four at most 4096 */
  lastNl = mgBlockReduce<CP_THREADS, MgMax> (lastNl, s64);
  if (threadIdx.x == 0) { tileNl[blockIdx.x] = total; tileLastNl[blockIdx.x] = lastNl; tileCnt[blockIdx.x] = cnt; }
}

/* Q2 */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgCompLineScanKernel (const U32 *__restrict__ tileNl, U64 *tileLastNl, const U64 *__restrict__ tileCnt, U64 nTiles, U64 *tileLine, U64 *tileDiff, int edge, CpState *st)      /* edge: 0 the text's first window, 1 the byte before the window is a newline, 2 it is not */
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U64 nlBefore = st->nl;
  const U64 nl = mgGroupScan<MgSum> (tileNl, tileLine, nTiles, nlBefore, lds);
  const U64 lastNl = mgGroupScan<MgMax> (tileLastNl, tileLastNl, nTiles, st->lastNl, lds);
  __syncthreads ();
  for (U64 t = threadIdx.x ; t < nTiles ; t += MG_GROUP_THREADS)
    { const U32 phase = (U32) tileLine[t] & 3u;             /* of the tile's first byte: the tile's lines 1 - phase and 3 - phase (mod 4) are sequence and quality lines */
      const U64 c = tileCnt[t];
      const U32 seq = (U32) (c >> (16 * ((1u - phase) & 3u))) & 0xffffu, qual = (U32) (c >> (16 * ((3u - phase) & 3u))) & 0xffffu;
      tileDiff[t] = (U64) (int64_t) ((int) seq - (int) qual);
    }
  __syncthreads ();
  const U64 diff = mgGroupScan<MgSum> (tileDiff, tileDiff, nTiles, st->diff, lds);
  if (threadIdx.x == 0)
    { if (edge == 2 || (edge == 1 && (nlBefore & 3u))) ++st->crossed;      /* the window begins inside a record */
      st->nl = nl; st->lastNl = lastNl; st->diff = diff;
    }
}

/* Q3 */
__global__ __launch_bounds__ (CP_THREADS)
void mgCompFastqKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 prevByte, U64 nTiles,
                        const U64 *__restrict__ tileLine, const U64 *__restrict__ tileLastNl, const U64 *__restrict__ tileDiff,
                        U32 *__restrict__ tileMinE, U64 *__restrict__ tileMinM, int flags, CpBins bins, CpState *st)
{
  __shared__ U32 sHistB[CP_HISTS][256], sHistQ[CP_HISTS][256];
  __shared__ U64 sAcc[CP_S_COUNT];
  __shared__ U64 s64[CP_WAVES];
  __shared__ U32 s32[CP_WAVES];
  for (U32 i = threadIdx.x ; i < CP_HISTS * 256 ; i += CP_THREADS) { (&sHistB[0][0])[i] = 0; (&sHistQ[0][0])[i] = 0; }
  if (threadIdx.x < CP_S_COUNT) sAcc[threadIdx.x] = 0;
  __syncthreads ();
  U32 *histB = sHistB[CP_HIST_MODE ? threadIdx.x >> 6 : 0], *histQ = sHistQ[CP_HIST_MODE ? threadIdx.x >> 6 : 0];
  for (U64 tile = blockIdx.x ; tile < nTiles ; tile += gridDim.x)
    { const U64 at = (tile * CP_THREADS + threadIdx.x) * 16;
      unsigned char b[16]; U32 prev0 = 0, nl = 0; U64 myLastNl = 0;
      if (at < n)
        { txLoad (text, n, at, prevByte, b, &prev0);
          nl = txNewlines (b, at, n);
#pragma unroll
          for (int j = 0 ; j < 16 ; ++j) if (at + j < n && b[j] == '\n') myLastNl = textBase + at + j + 1;
        }
      U32 total;
      U64 line = tileLine[tile] + (mgBlockInclusive<CP_THREADS, MgSum> (nl, s32, &total) - nl);        /* newlines of the text before the thread's first byte */
      const U64 nlExcl = mgBlockExclusive<CP_THREADS, MgMax> (myLastNl, s64);
      U64 prevNl = nlExcl > tileLastNl[tile] ? nlExcl : tileLastNl[tile];                                  /* position + 1 of the last of them */
      /* the thread's sequence-line bytes less its quality-line bytes: its place in the running difference (within +-4096 inside a tile) */
      U32 d = 0;
      if (at < n)
        { U32 l = (U32) line;
#pragma unroll
          for (int j = 0 ; j < 16 ; ++j)
            if (at + j < n) { if (b[j] == '\n') ++l; else if ((l & 3u) == 1u) ++d; else if ((l & 3u) == 3u) --d; }
        }
      U64 diff = tileDiff[tile] + (U64) (int64_t) (int) (mgBlockInclusive<CP_THREADS, MgSum> (d, s32, &total) - d);
      CpAcc a = { 0, 0, 0, 0, CP_NONE };
      if (at < n)
        { U32 prev = prev0;
          U64 errLine = CP_NONE, bad = CP_NONE, badLine = CP_NONE, lastEnd = 0;
          CpRun hb = { 0, 0 }, hq = { 0, 0 };
#pragma unroll
          for (int j = 0 ; j < 16 ; ++j)
            { if (at + j < n)
                { const U32 c = b[j];
                  const U32 phase = (U32) line & 3u;
                  const U64 pos = textBase + at + j;
                  if (prev == '\n' && ((phase == 0 && c != '@') || (phase == 2 && c != '+')) && errLine == CP_NONE) errLine = line + 1;      /* seqio.c:302,333 */
                  if (c == '\n')
                    { if (phase == 3)
                        { if (diff && errLine == CP_NONE) errLine = line + 1;             /* seqio.c:338: the first record whose two lines differ */
                          cpRecord (a, pos - prevNl, bins, st);
                          lastEnd = pos + 2;
                        }
                      prevNl = pos + 1; ++line;
                    }
                  else if (phase == 1)
                    { ++diff;
                      if (flags & MG_COMP_BASES)
                        { if (c >= 0x80u) { if (bad == CP_NONE) { bad = pos; badLine = line + 1; } }      /* totBase[*s++] with a char (composition.c:61) */
                          else cpHistAdd (histB, hb, c);
                        }
                    }
                  else if (phase == 3)
                    { --diff;
                      if (flags & MG_COMP_QUALS)
                        { if (c < 33u || c >= 0x80u) { if (bad == CP_NONE) { bad = pos; badLine = line + 1; } }      /* totQual[*q++] after -= 33 (seqio.c:340, composition.c:71) */
                          else cpHistAdd (histQ, hq, c - 33u);
                        }
                    }
                }
              prev = b[j];
            }
          cpHistFlush (histB, hb); cpHistFlush (histQ, hq);
          if (errLine != CP_NONE) cpMin64 (&st->errLine, errLine);
          if (bad != CP_NONE) { cpMin64 (&st->badOff, bad); cpMin64 (&st->badLine, badLine); }
          if (lastEnd) cpMax64 (&sAcc[CP_S_LASTSTART], lastEnd);
        }
      cpTileOut (a, sAcc, s32, s64, tile, tileMinE, tileMinM);
    }
  __syncthreads ();
  if (flags & MG_COMP_BASES) cpHistOut (sHistB, st->base);
  if (flags & MG_COMP_QUALS) cpHistOut (sHistQ, st->qual);
  cpAccOut (sAcc, st);
}

/* Q4 */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgCompFastqPairKernel (U64 nTiles, const U32 *__restrict__ tileMinE, const U64 *__restrict__ tileMinM, CpState *st)
{
  __shared__ U64 lds[MG_GROUP_THREADS / 64];
  cpFoldPairs (nTiles, tileMinE, tileMinM, st, lds);
}

/* ---------------------------------------------------------------------------------------- */
/* host side                                                                                  */

static thread_local U64 gCompDiag[4];                    /* windows, tiles, records across a window edge, kernel launches */
extern "C" void mgCompositionDiag (U64 out4[4]) { memcpy (out4, gCompDiag, sizeof (gCompDiag)); }

struct CpPass {                                          /* one walk over the text */
  int flags = 0, type = 0;
  size_t tilesCap = 0;
  CpState *dState = 0;
  U64 *dA = 0, *dB = 0, *dC = 0, *dD = 0, *dMinM = 0;     /* per tile, 64-bit: FASTA events, kept offsets, last-start codes; FASTQ lines, last newlines, differences, counts */
  U32 *dU = 0, *dV = 0, *dW = 0, *dMinE = 0;              /* per tile, 32-bit */
  CpBins bins = { 0, 0, 0 };
  U32 lastByte = 0; U64 bytes = 0;
  bool typeError = false;
  ~CpPass () { (void) hipFree (bins.count); (void) hipFree (bins.sum); }
  /* the bins the records of the text so far can reach: a record is no longer than the text */
  int growBins (U64 textEnd)
  { if (!(flags & MG_COMP_LENGTHS)) return 0;
    const U64 reach = textEnd < CP_MAXLEN ? textEnd : CP_MAXLEN;
    const U64 need = (U64) sqrt (100.0 * (double) reach) + 4;
    if (need <= bins.cap) return 0;
    const U64 cap = need > 2 * bins.cap ? need : 2 * bins.cap;
    U32 *c = 0; U64 *s = 0;
    if (hipMalloc ((void **) &c, cap * 4) != hipSuccess || hipMalloc ((void **) &s, cap * 8) != hipSuccess
        || hipMemset (c, 0, cap * 4) != hipSuccess || hipMemset (s, 0, cap * 8) != hipSuccess
        || (bins.cap && (hipMemcpy (c, bins.count, bins.cap * 4, hipMemcpyDeviceToDevice) != hipSuccess || hipMemcpy (s, bins.sum, bins.cap * 8, hipMemcpyDeviceToDevice) != hipSuccess)))
      { (void) hipFree (c); (void) hipFree (s); mgHipFail (hipGetLastError (), "mgComposition"); return -1; }
    (void) hipFree (bins.count); (void) hipFree (bins.sum);
    bins.count = c; bins.sum = s; bins.cap = cap;
    return 0;
  }
  static int window (void *v, const MgTextWindow *w, void *stream)
  { CpPass *p = (CpPass *) v;
    hipStream_t st = (hipStream_t) stream;
    if (!w->index)
      { p->type = w->first == '>' ? 1 : w->first == '@' ? 2 : 0;
        if (!p->type) { p->typeError = true; return -1; }
      }
    const U64 nTiles = (w->n + CP_TILE - 1) / CP_TILE;
    if (nTiles > p->tilesCap) { mgSetError ("mgComposition: a window of %llu tiles, room for %llu", (unsigned long long) nTiles, (unsigned long long) p->tilesCap); return -1; }
    if (p->growBins (w->off + w->n)) return -1;
    const unsigned grid = (unsigned) (nTiles < CP_GRID ? nTiles : CP_GRID);
    if (p->type == 1)
      { if (mgTextLaunchEventTiles (w->dText, w->n, w->off, w->prevByte, p->dA, stream)) return mgFailedWith ("mgComposition: launch failed");
        hipLaunchKernelGGL (mgCompStateScanKernel, dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, p->dA, nTiles, p->dState);
        hipLaunchKernelGGL (mgCompFastaKernel, dim3 (grid), dim3 (CP_THREADS), 0, st, w->dText, (U64) w->n, w->off, w->prevByte, nTiles, p->dA,
                            p->dU, p->dV, p->dW, p->dMinE, p->dMinM, p->flags, p->bins, p->dState);
        const int crossing = w->index && !(w->first == '>' && w->prevByte == '\n');
        hipLaunchKernelGGL (mgCompFastaStitchKernel, dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, nTiles, p->dU, p->dV, p->dW, p->dMinE, p->dMinM, p->dB, p->dC, crossing, p->bins, p->dState);
      }
    else
      { hipLaunchKernelGGL (mgCompLinesKernel, dim3 ((unsigned) nTiles), dim3 (CP_THREADS), 0, st, w->dText, (U64) w->n, w->off, p->dU, p->dB, p->dD);
        hipLaunchKernelGGL (mgCompLineScanKernel, dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, p->dU, p->dB, p->dD, nTiles, p->dA, p->dC, !w->index ? 0 : w->prevByte == '\n' ? 1 : 2, p->dState);
        hipLaunchKernelGGL (mgCompFastqKernel, dim3 (grid), dim3 (CP_THREADS), 0, st, w->dText, (U64) w->n, w->off, w->prevByte, nTiles, p->dA, p->dB, p->dC,
                            p->dMinE, p->dMinM, p->flags, p->bins, p->dState);
        hipLaunchKernelGGL (mgCompFastqPairKernel, dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, nTiles, p->dMinE, p->dMinM, p->dState);
      }
    if (hipGetLastError () != hipSuccess) return mgFailedWith ("mgComposition: launch failed");
    p->lastByte = w->last; p->bytes = w->off + w->n;
    gCompDiag[1] += nTiles; gCompDiag[3] += 4;
    return 0;
  }
};

struct CpResult { CpState st; std::vector<U32> binCount; std::vector<U64> binSum; int type = 0; U32 lastByte = 0; };

static U64 cpIsqrtHost (U64 x) { U64 r = (U64) sqrt ((double) x); while (r * r > x) --r; while ((r + 1) * (r + 1) <= x) ++r; return r; }

/* the text of `src` below src.limit through the kernels; 0 / -1 */
static int cpWalk (CpSource &src, int flags, int force, CpResult *out)
{
  MgDevScratch scratch ("mgComposition");
  CpPass p; p.flags = flags;
  p.tilesCap = mgTextWindowBytes ((size_t) src.size) / CP_TILE + 2;
  U64 **a64[5] = { &p.dA, &p.dB, &p.dC, &p.dD, &p.dMinM }; U32 **a32[4] = { &p.dU, &p.dV, &p.dW, &p.dMinE };
  if (scratch.get (&p.dState, 1)) return -1;
  for (int i = 0 ; i < 5 ; ++i) if (scratch.get (a64[i], p.tilesCap)) return -1;
  for (int i = 0 ; i < 4 ; ++i) if (scratch.get (a32[i], p.tilesCap)) return -1;
  memset (&out->st, 0, sizeof (CpState));
  out->st.minM = out->st.errLine = out->st.badOff = out->st.badLine = CP_NONE;
  if (hipMemcpy (p.dState, &out->st, sizeof (CpState), hipMemcpyHostToDevice) != hipSuccess) { scratch.fail (); return -1; }
  if (!src.stream () && p.growBins (src.size < src.limit ? src.size : src.limit)) return -1;
  U64 nWindows = 0;
  const int rc = src.walk ((size_t) src.size, CpSource::fill, CpPass::window, &p, &nWindows);
  gCompDiag[0] += nWindows;
  if (p.typeError) { mgSetError ("sequence file %s is neither FASTA nor FASTQ text", src.name ? src.name : "(text)"); return -1; }
  if (rc) return -1;
  if (!nWindows) { mgSetError ("sequence file %s unreadable or empty", src.name ? src.name : "(text)"); return -1; }
  if (p.type == 1)
    { hipLaunchKernelGGL (mgCompFastaFinishKernel, dim3 (1), dim3 (64), 0, (hipStream_t) 0, p.lastByte, p.bytes, force, p.bins, p.dState);
      ++gCompDiag[3];
    }
  if (hipMemcpy (&out->st, p.dState, sizeof (CpState), hipMemcpyDeviceToHost) != hipSuccess) { scratch.fail (); return -1; }
  out->type = p.type; out->lastByte = p.lastByte;
  gCompDiag[2] += out->st.crossed;
  if (p.type == 2) out->st.complete = force || (p.lastByte == '\n' && !(out->st.nl & 3)) ? 1 : 0;
  if (out->st.binOverflow) { mgSetError ("mgComposition: a record beyond the length bins"); return -1; }
  if ((flags & MG_COMP_LENGTHS) && out->st.nSeq && !out->st.tooLong)
    { const U64 nBins = cpIsqrtHost (100 * out->st.lenMax) + 1;                /* the arrays' extent: the largest bin touched, plus 1 (array.h) */
      if (nBins > p.bins.cap) { mgSetError ("mgComposition: a record beyond the length bins"); return -1; }
      out->binCount.resize (nBins); out->binSum.resize (nBins);
      if (hipMemcpy (out->binCount.data (), p.bins.count, nBins * 4, hipMemcpyDeviceToHost) != hipSuccess
          || hipMemcpy (out->binSum.data (), p.bins.sum, nBins * 8, hipMemcpyDeviceToHost) != hipSuccess) { scratch.fail (); return -1; }
    }
  return 0;
}

static void cpAppend (std::string &s, const char *fmt, ...)
{
  char buf[256]; va_list ap; va_start (ap, fmt); vsnprintf (buf, sizeof (buf), fmt, ap); va_end (ap); s += buf;
}

/* composition.c:74-117 with the reference's format strings and its arithmetic */
static void cpPrint (std::string &s, int flags, const MgComposition *r)
{
  typedef unsigned long long ull;
  const U64 totLen = r->totLen;
  cpAppend (s, "%s file, %llu sequences >= 0, %llu total, %.2f average, %llu min, %llu max\n", r->type == 1 ? "fasta" : "fastq",
            (ull) r->nSeq, (ull) totLen, totLen / (double) r->nSeq, (ull) r->lenMin, (ull) r->lenMax);
  if (flags & MG_COMP_BASES)
    { U64 totUnprint = 0;
      s += "bases\n";
      for (int i = 0 ; i < 256 ; ++i)
        if (r->base[i])
          { if (i >= 0x20 && i < 0x7f) cpAppend (s, "  %c %llu %4.1f %%\n", i, (ull) r->base[i], r->base[i] * 100.0 / totLen);      /* isprint in the C locale */
            else totUnprint += r->base[i];
          }
      if (totUnprint) cpAppend (s, " unprintable %llu %4.1f %%\n", (ull) totUnprint, totUnprint * 100.0 / totLen);
    }
  if ((flags & MG_COMP_QUALS) && r->type == 2)
    { s += "qualities\n";
      U64 sum = 0;
      for (int i = 0 ; i < 256 ; ++i)
        { sum += r->qual[i];
          if (r->qual[i]) cpAppend (s, " %3d %llu %4.1f %% %5.1f %%\n", i, (ull) r->qual[i], r->qual[i] * 100.0 / totLen, sum * 100.0 / totLen);
        }
    }
  if ((flags & MG_COMP_LENGTHS) && r->lenMin < r->lenMax)
    { const int nBins = (int) r->nBins;
      U64 tot50 = 0;
      int i;
      for (i = 0 ; i < nBins && tot50 < 0.5 * totLen ; ++i) tot50 += r->binSum[i];
      cpAppend (s, "approximate N50 %d\n", (int) ((unsigned) i * (unsigned) (i + 1)) / 100);
      s += "length distribution (quadratic bins)\n";
      int sum = 0;
      const int d = nBins / 20;
      for (i = 0 ; i < nBins ; ++i)
        { sum += r->binCount[i];
          if (sum && !((nBins - 1 - i) % d)) { cpAppend (s, "  %d\t%d\n", (int) ((unsigned) i * (unsigned) i) / 100, sum); sum = 0; }
        }
    }
}

static int cpCompose (CpSource &src, int flags, FILE *out, FILE *err, MgComposition *res)
{
  typedef unsigned long long ull;
  memset (gCompDiag, 0, sizeof (gCompDiag)); mgInflateDiagReset (); mgGunzipDiagReset ();
  if (res) memset (res, 0, sizeof (*res));
  if (flags & ~(MG_COMP_BASES | MG_COMP_QUALS | MG_COMP_LENGTHS)) { mgSetError ("mgComposition: unknown flags %d", flags); return -1; }
  if (mgEnsureDevice ()) return -1;
  CpResult w;
  if (cpWalk (src, flags, 0, &w)) return -1;
  const CpState &S = w.st;
  /* what the reference die()s on, and the bytes it would index a table out of bounds with: whichever comes first, record by record -- a
     record's rules are checked when it is read, its bytes are counted after that */
  const bool rule = S.errLine != CP_NONE, bad = S.badOff != CP_NONE;
  const U64 ruleRec = rule ? (S.errLine - 1) / 4 : 0, badRec = w.type == 2 && bad ? (S.badLine - 1) / 4 : 0;
  if (rule && (!bad || ruleRec <= badRec))
    { const char *what = (S.errLine & 3) == 1 ? "no initial @ for FASTQ record line" : (S.errLine & 3) == 3 ? "missing + FASTQ line" : "qual not same length as seq line";
      mgSetError ("%s %llu", what, (ull) S.errLine);
      return -1;
    }
  const U64 cut = S.lastStart ? S.lastStart - 1 : 0;       /* where the text's last record starts (FASTA) / the byte after its last complete one (FASTQ) */
  if (bad && (S.complete || rule || (w.type == 1 ? S.badOff < cut : badRec < S.nSeq)))
    { mgSetError ("byte at offset %llu of the %s is outside the reference's tables (composition would index them out of bounds)", (ull) S.badOff,
                  w.type == 1 ? "FASTA sequence lines" : "FASTQ record lines");
      return -1;
    }
  std::string errText;
  if (!S.complete)                                           /* seqio.c:215-219: the record is dropped, the ones before it are reported */
    { char line[96]; snprintf (line, sizeof (line), "incomplete sequence record line %llu\n", (ull) ((w.type == 1 ? S.newlines : S.nl) + 1));
      errText = line;
      const int type = w.type;
      if (cut)
        { src.limit = cut;
          if (src.reopen () || cpWalk (src, flags, 1, &w)) return -1;
        }
      else { w = CpResult (); memset (&w.st, 0, sizeof (CpState)); w.st.minM = CP_NONE; w.type = type; }
    }
  if (w.st.tooLong) { mgSetError ("a record of 2^31 bases or more: the reference's lengths are int"); return -1; }
  MgComposition r; memset (&r, 0, sizeof (r));
  r.type = w.type; r.nSeq = w.st.nSeq; r.totLen = w.st.totLen; r.lenMax = w.st.lenMax; r.lenMin = w.st.minM == CP_NONE ? 0 : w.st.minM;
  memcpy (r.base, w.st.base, sizeof (r.base)); memcpy (r.qual, w.st.qual, sizeof (r.qual));
  if ((flags & MG_COMP_LENGTHS) && !w.binCount.empty ())
    { r.nBins = (U32) w.binCount.size ();
      r.binCount = (int *) malloc (r.nBins * sizeof (int)); r.binSum = (U64 *) malloc (r.nBins * sizeof (U64));
      if (!r.binCount || !r.binSum) { free (r.binCount); free (r.binSum); mgSetError ("mgComposition: out of memory"); return -1; }
      for (U32 i = 0 ; i < r.nBins ; ++i) { r.binCount[i] = (int) w.binCount[i]; r.binSum[i] = w.binSum[i]; }
    }
  int rc = 0;
  if ((flags & MG_COMP_LENGTHS) && r.lenMin < r.lenMax && r.nBins / 20 == 0)
    { mgSetError ("-l with every record shorter than 4 bases: the reference divides by zero (composition.c:107,110: %u bins / 20)", r.nBins); rc = -1; }
  else
    { std::string text;
      cpPrint (text, flags, &r);
      if (out) fwrite (text.data (), 1, text.size (), out);
      if (err && !errText.empty ()) fwrite (errText.data (), 1, errText.size (), err);
    }
  if (res) *res = r; else { free (r.binCount); free (r.binSum); }
  return rc;
}

extern "C" int mgCompositionFile (const char *filename, int flags, FILE *out, FILE *err, MgComposition *res)
{
  CpSource src;
  if (res) memset (res, 0, sizeof (*res));
  if (src.open (filename)) { src.close (); return -1; }
  const int rc = cpCompose (src, flags, out, err, res);
  src.close ();
  return rc;
}

extern "C" int mgCompositionText (const char *text, U64 n, int flags, FILE *out, FILE *err, MgComposition *res)
{
  CpSource src;
  if (res) memset (res, 0, sizeof (*res));
  if (!text || !n) { mgSetError ("sequence text unreadable or empty"); return -1; }
  src.mem = (const unsigned char *) text; src.size = n;
  return cpCompose (src, flags, out, err, res);
}

extern "C" void mgCompositionFree (MgComposition *res)
{
  if (!res) return;
  free (res->binCount); free (res->binSum);
  res->binCount = 0; res->binSum = 0; res->nBins = 0;
}
