/* mg_textparse.hip — the device text parser's kernels (FASTA: K1 .. K5 and K6 for a text of unknown size, FASTQ: Kq1 .. Kq6, the carry) and the ONE parse loop over the window walk,
 * with what differs between the two formats in FaFormat / FqFormat.  mg_textgpu.hip's file comment says what the kernels do and why. */
#include <stddef.h>
#include <string.h>
#include "mg_text_int.h"

#define TX_THREADS 256
static_assert (TX_THREADS * TX_PER == MG_TEXT_TILE, "mg_internal.h states the tile");
/* txLoad, txEvent, txLastEvent and txNewlines: mg_internal.h (mg_composition.hip reads text by the same rules) */

/* base code of a text byte, 4 = not a base (seqio.c:643-652 + N -> 0): branch-free on the letter */
__device__ __forceinline__ U32 txCode (U32 c)
{
  const U32 u = c & 0xdfu;                                /* upper case */
  U32 code = 4;
  code = u == 'A' ? 0u : code; code = u == 'C' ? 1u : code; code = u == 'G' ? 2u : code; code = u == 'T' ? 3u : code; code = u == 'N' ? 0u : code;
  return code;
}

/* K1: the last event of every tile */
__global__ __launch_bounds__ (TX_THREADS)
void mgTextEventKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 prevByte, U64 *__restrict__ tileEvent)
{
  __shared__ U64 sRed[TX_THREADS / 64];
  const U64 at = ((U64) blockIdx.x * TX_THREADS + threadIdx.x) * TX_PER;
  unsigned char b[16]; U32 prev = 0;
  U64 last = 0;
  if (at < n) { txLoad (text, n, at, prevByte, b, &prev); last = txLastEvent (b, at, n, prev, textBase + at); }
  const U64 m = mgBlockReduce<TX_THREADS, MgMax> (last, sRed);
  if (threadIdx.x == 0) tileEvent[blockIdx.x] = m;
}

/* K2: the running maximum over the tiles' events, on top of the state the window before ended in -> what holds at every tile's first byte */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgTextStateScanKernel (U64 *tileEvent, U64 nTiles, TxState *st)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U64 total = mgGroupScan<MgMax> (tileEvent, tileEvent, nTiles, st->lastEvent, lds);
  if (threadIdx.x == 0) st->lastEvent = total;            /* the state the next window starts in */
}

/* the state at a thread's first byte, for K3 and K5: from the tile's incoming event and the last events of the threads before it in the tile */
__device__ __forceinline__ U64 txIncoming (U64 myLast, U64 tileIn, U64 *sScan)
{
  const U64 excl = mgBlockExclusive<TX_THREADS, MgMax> (myLast, sScan);      /* the last event of the threads before this one */
  return excl > tileIn ? excl : tileIn;
}
/* the walk over a thread's 16 bytes, shared by K3 and K5: EMIT = false counts bases and record starts, EMIT = true writes them */
template <bool EMIT>
__device__ __forceinline__ void faWalk (const unsigned char *b, U64 at, U64 n, U32 prev, bool header, U64 filePos, U32 *nb, U32 *ns,
                                        unsigned char *bases, U64 myB, U64 *recOff, U64 *recPos, U64 myS)
{
  U32 cb = 0, cs = 0;      /* (counted here and stored once: counters bumped through the pointers end up in scratch memory) */
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j)
    { if (at + j < n)
        { const U32 c = b[j];
          if (c == '>' && prev == '\n')
            { header = true;
              if (EMIT) { if (recPos) recPos[myS] = filePos + (U64) j; recOff[myS++] = myB; }      /* a record's offset: the bases before its '>' */
              else ++cs;
            }
          else if (c == '\n') header = false;
          else if (!header && txCode (c) < 4) { if (EMIT) bases[myB++] = (unsigned char) txCode (c); else ++cb; }
        }
      prev = b[j];
    }
  if (!EMIT) { *nb = cb; *ns = cs; }
}

/* K3: bases and record starts of every tile */
__global__ __launch_bounds__ (TX_THREADS)
void mgTextCountKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 prevByte, const U64 *__restrict__ tileIn,
                        U32 *__restrict__ tileBases, U32 *__restrict__ tileStarts)
{
  __shared__ U64 sScan[TX_THREADS / 64];
  __shared__ U32 sRed[TX_THREADS / 64];
  const U64 at = ((U64) blockIdx.x * TX_THREADS + threadIdx.x) * TX_PER;
  unsigned char b[16]; U32 prev = 0;
  U64 last = 0;
  if (at < n) { txLoad (text, n, at, prevByte, b, &prev); last = txLastEvent (b, at, n, prev, textBase + at); }
  const bool header = (txIncoming (last, tileIn[blockIdx.x], sScan) & 1) != 0;
  U32 nb = 0, ns = 0;
  if (at < n) faWalk<false> (b, at, n, prev, header, 0, &nb, &ns, 0, 0, 0, 0, 0);
  nb = mgBlockReduce<TX_THREADS, MgSum> (nb, sRed); ns = mgBlockReduce<TX_THREADS, MgSum> (ns, sRed);
  if (threadIdx.x == 0) { tileBases[blockIdx.x] = nb; tileStarts[blockIdx.x] = ns; }
}

/* K4: where every tile's bases and record offsets go in the batch accumulator; the new totals */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgTextOffsetScanKernel (const U32 *__restrict__ tileBases, const U32 *__restrict__ tileStarts, U64 nTiles,
                             U64 *__restrict__ tileBaseOff, U64 *__restrict__ tileStartOff, TxState *st, U64 *hostCounts)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U64 totB = mgGroupScan<MgSum> (tileBases, tileBaseOff, nTiles, st->accBases, lds);
  const U64 totS = mgGroupScan<MgSum> (tileStarts, tileStartOff, nTiles, st->accRecs, lds);
  if (threadIdx.x == 0)
    { st->accBases = totB; st->accRecs = totS;
      hostCounts[0] = totB; hostCounts[1] = totS;           /* pinned host words: the host decides about the batch from them */
    }
}

/* K5: the bases (one byte each) and the record offsets, written where the sums say */
__global__ __launch_bounds__ (TX_THREADS)
void mgTextEmitKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 prevByte,
                       const U64 *__restrict__ tileIn, const U64 *__restrict__ tileBaseOff, const U64 *__restrict__ tileStartOff,
                       unsigned char *__restrict__ bases, U64 basesCap, U64 *__restrict__ recOff, U64 recCap, U32 *__restrict__ overflow,
                       U64 *__restrict__ recPos)      /* != 0: the file position of every record's '>' (the callers that print record ids) */
{
  __shared__ U64 sScan[TX_THREADS / 64];
  __shared__ U32 sRed[TX_THREADS / 64];
  const U64 at = ((U64) blockIdx.x * TX_THREADS + threadIdx.x) * TX_PER;
  unsigned char b[16]; U32 prev = 0;
  U64 last = 0;
  if (at < n) { txLoad (text, n, at, prevByte, b, &prev); last = txLastEvent (b, at, n, prev, textBase + at); }
  const bool header = (txIncoming (last, tileIn[blockIdx.x], sScan) & 1) != 0;
  /* the thread's counts (its place inside the tile), then the walk that writes */
  U32 nb = 0, ns = 0;
  if (at < n) faWalk<false> (b, at, n, prev, header, 0, &nb, &ns, 0, 0, 0, 0, 0);
  const U64 myB = tileBaseOff[blockIdx.x] + mgBlockExclusive<TX_THREADS, MgSum> (nb, sRed);
  const U64 myS = tileStartOff[blockIdx.x] + mgBlockExclusive<TX_THREADS, MgSum> (ns, sRed);
  if (!nb && !ns) return;
  if (myB + nb > basesCap || myS + ns > recCap) { *overflow = 1; return; }
  faWalk<true> (b, at, n, prev, header, textBase + at, 0, 0, bases, myB, recOff, recPos, myS);
}

/* the carried record moves to the front of the accumulator (regions may overlap: chunks in order, one workgroup) */
__global__ __launch_bounds__ (1024)
void mgTextCarryKernel (unsigned char *bases, U64 from, U64 count)
{
  for (U64 i0 = 0 ; i0 < count ; i0 += 1024)
    { const U64 i = i0 + threadIdx.x;
      unsigned char v = 0;
      if (i < count) v = bases[from + i];
      __syncthreads ();
      if (i < count) bases[i] = v;
      __syncthreads ();
    }
}

/* ... and when the regions do not overlap (the carried record is shorter than what was handed on: always, unless one record is longer than a
   whole batch) the move is a plain copy by the whole chip -- the one-workgroup form took 6 ms per carry of a 100 Mbp chromosome, a quarter of a
   reference file's read (tools/longfile_trace.sh) */
__global__ __launch_bounds__ (256)
void mgTextCarryWideKernel (unsigned char *bases, U64 from, U64 count)
{
  const U64 stride = (U64) gridDim.x * blockDim.x * 4;
  for (U64 i = ((U64) blockIdx.x * blockDim.x + threadIdx.x) * 4 ; i < count ; i += stride)
    { if (i + 4 <= count && !((from + i) & 3))
        *reinterpret_cast<U32 *> (bases + i) = *reinterpret_cast<const U32 *> (bases + from + i);
      else
        for (int j = 0 ; j < 4 && i + j < count ; ++j) bases[i + j] = bases[from + i + j];
    }
}
static void txCarry (unsigned char *bases, U64 from, U64 count, hipStream_t st)
{
  if (!count) return;
  if (count <= from)
    { unsigned grid = (unsigned) ((count / 4 + 255) / 256); if (grid > 8192) grid = 8192; if (!grid) grid = 1;
      hipLaunchKernelGGL (mgTextCarryWideKernel, dim3 (grid), dim3 (256), 0, st, bases, from, count);
    }
  else hipLaunchKernelGGL (mgTextCarryKernel, dim3 (1), dim3 (1024), 0, st, bases, from, count);
}

/* ======================================================================================== */
/* FASTQ: four lines a record (seqio.c:325-339).  The line a byte belongs to is the number of newlines before it, a prefix
 * sum; line mod 4 says what the byte is: 0 header ('@' first), 1 sequence (EVERY byte but the newline is a base: A/a C/c G/g
 * T/t N/n as in FASTA, anything else stays in the sequence as (char) -2, i.e. 2 once packed -- as the host parser and the
 * reference leave it), 2 the '+' line, 3 qualities (as many bytes as the sequence line).  A record is complete at its fourth
 * newline; there the kernels note the bases and the quality bytes counted so far and the newline's file position: the first
 * gives the read offsets, the first two the length check, the third where the host parser would take over.  The rules
 * ('@', '+', equal lengths, whole records at the end of the file) are CHECKED here and never judged: any breach, and the file
 * goes back to the host parser from the first record not yet added, which then says what the reference says. */

/* Kq1: newlines per tile */
__global__ __launch_bounds__ (TX_THREADS)
void mgTextNewlineKernel (const unsigned char *__restrict__ text, U64 n, U64 *__restrict__ tileNL)
{
  __shared__ U32 sRed[TX_THREADS / 64];
  const U64 at = ((U64) blockIdx.x * TX_THREADS + threadIdx.x) * TX_PER;
  unsigned char b[16]; U32 prev = 0; U32 c = 0;
  if (at < n)
    { txLoad (text, n, at, 0, b, &prev);
      c = txNewlines (b, at, n);
    }
  const U32 t = mgBlockReduce<TX_THREADS, MgSum> (c, sRed);
  if (threadIdx.x == 0) tileNL[blockIdx.x] = t;
}

/* Kq2: the line number at every tile's first byte */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgTextLineScanKernel (U64 *tileNL, U64 nTiles, TqState *st)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U64 total = mgGroupScan<MgSum> (tileNL, tileNL, nTiles, st->nlCount, lds);
  if (threadIdx.x == 0) st->nlCount = total;
}

/* K6, FASTA out of a source that does not know its text's size: the line number of the last record start so far -- 1 + the newlines before its '>' --
   which the hand-over of a text that ends in an unfinished record names.  Behind Kq1 and Kq2 over the same window (tileLine: the newlines before every
   tile) and K5 (recPos); one workgroup, over the tile that holds the '>'.  A record that started windows ago keeps the number it got then. */
__global__ __launch_bounds__ (TX_THREADS)
void mgTextRecordLineKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, const U64 *__restrict__ recPos, U64 lastRec,
                             const U64 *__restrict__ tileLine, U64 *__restrict__ openLine)
{
  __shared__ U32 sRed[TX_THREADS / 64];
  const U64 p = recPos[lastRec] - textBase;               /* (the record starts in this window: p < n) */
  if (p >= n) return;
  const U64 tile = p / TX_TILE, at = (tile * TX_THREADS + threadIdx.x) * TX_PER;
  unsigned char b[16]; U32 prev = 0, c = 0;
  if (at < p)
    { txLoad (text, n, at, 0, b, &prev);
      c = txNewlines (b, at, p);                           /* the newlines of the tile before byte p */
    }
  const U32 before = mgBlockReduce<TX_THREADS, MgSum> (c, sRed);
  if (threadIdx.x == 0) *openLine = tileLine[tile] + before + 1;
}

/* the walk over a thread's 16 bytes, shared by Kq3 (counts) and Kq5 (writes): EMIT = false counts only */
template <bool EMIT>
__device__ __forceinline__ void tqWalk (const unsigned char *b, U64 at, U64 n, U32 prev, U64 line, U64 filePos,
                                        U32 *nb, U32 *nq, U32 *ne, U32 *bad,
                                        unsigned char *bases, U64 myB, U64 myQ, U64 *endB, U64 *endQ, U64 *endP, U64 myE)
{
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j)
    { if (at + j < n)
        { const U32 c = b[j];
          const U32 phase = (U32) line & 3u;
          if (prev == '\n' && ((phase == 0 && c != '@') || (phase == 2 && c != '+'))) *bad = 1;     /* seqio.c:326,333 */
          if (c == '\n')
            { if (phase == 3)
                { if (EMIT) { endB[myE] = myB; endQ[myE] = myQ; endP[myE] = filePos + (U64) j; ++myE; }
                  ++*ne;
                }
              ++line;
            }
          else if (phase == 1) { if (EMIT) { const U32 code = txCode (c); bases[myB++] = (unsigned char) (code < 4 ? code : 2u); } ++*nb; }
          else if (phase == 3) { if (EMIT) ++myQ; ++*nq; }
        }
      prev = b[j];
    }
}

/* Kq3: bases, quality bytes and completed records of every tile; rule checks at the line starts */
__global__ __launch_bounds__ (TX_THREADS)
void mgTextFastqCountKernel (const unsigned char *__restrict__ text, U64 n, U32 prevByte, const U64 *__restrict__ tileLine,
                             U32 *__restrict__ tileBases, U32 *__restrict__ tileQual, U32 *__restrict__ tileEnds, TqState *st)
{
  __shared__ U32 sScan[TX_THREADS / 64], sRed[TX_THREADS / 64];
  const U64 at = ((U64) blockIdx.x * TX_THREADS + threadIdx.x) * TX_PER;
  unsigned char b[16]; U32 prev = 0; U32 nl = 0;
  if (at < n)
    { txLoad (text, n, at, prevByte, b, &prev);
      nl = txNewlines (b, at, n);
    }
  const U64 line = tileLine[blockIdx.x] + mgBlockExclusive<TX_THREADS, MgSum> (nl, sScan);
  U32 nb = 0, nq = 0, ne = 0, bad = 0;
  if (at < n) tqWalk<false> (b, at, n, prev, line, 0, &nb, &nq, &ne, &bad, 0, 0, 0, 0, 0, 0, 0);
  if (bad) st->bad = 1;
  const U32 tb = mgBlockReduce<TX_THREADS, MgSum> (nb, sRed), tq = mgBlockReduce<TX_THREADS, MgSum> (nq, sRed), te = mgBlockReduce<TX_THREADS, MgSum> (ne, sRed);
  if (threadIdx.x == 0) { tileBases[blockIdx.x] = tb; tileQual[blockIdx.x] = tq; tileEnds[blockIdx.x] = te; }
}

/* Kq4: where the tiles' bases / quality counts / record ends go; the new totals */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgTextFastqOffsetKernel (const U32 *__restrict__ tileBases, const U32 *__restrict__ tileQual, const U32 *__restrict__ tileEnds, U64 nTiles,
                              U64 *__restrict__ offB, U64 *__restrict__ offQ, U64 *__restrict__ offE, TqState *st, U64 *hostCounts)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U64 totB = mgGroupScan<MgSum> (tileBases, offB, nTiles, st->accBases, lds);
  const U64 totQ = mgGroupScan<MgSum> (tileQual, offQ, nTiles, st->accQual, lds);
  const U64 totE = mgGroupScan<MgSum> (tileEnds, offE, nTiles, st->accRecs, lds);
  if (threadIdx.x == 0)
    { st->accBases = totB; st->accQual = totQ; st->accRecs = totE;
      hostCounts[0] = totB; hostCounts[1] = totE; hostCounts[2] = totQ; hostCounts[3] = st->nlCount; hostCounts[4] = st->bad;
    }
}

/* Kq5: the bases, and at every record's last newline the three running values (entries 1 .. of endB / endQ / endP; entry 0 is
 * what held when the accumulator was started) */
__global__ __launch_bounds__ (TX_THREADS)
void mgTextFastqEmitKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 prevByte, const U64 *__restrict__ tileLine,
                            const U64 *__restrict__ offB, const U64 *__restrict__ offQ, const U64 *__restrict__ offE,
                            unsigned char *__restrict__ bases, U64 basesCap, U64 *__restrict__ endB, U64 *__restrict__ endQ, U64 *__restrict__ endP, U64 recCap,
                            U32 *__restrict__ overflow)
{
  __shared__ U32 sScan[TX_THREADS / 64];
  const U64 at = ((U64) blockIdx.x * TX_THREADS + threadIdx.x) * TX_PER;
  unsigned char b[16]; U32 prev = 0; U32 nl = 0;
  if (at < n)
    { txLoad (text, n, at, prevByte, b, &prev);
      nl = txNewlines (b, at, n);
    }
  const U64 line = tileLine[blockIdx.x] + mgBlockExclusive<TX_THREADS, MgSum> (nl, sScan);
  U32 nb = 0, nq = 0, ne = 0, bad = 0;
  if (at < n) tqWalk<false> (b, at, n, prev, line, 0, &nb, &nq, &ne, &bad, 0, 0, 0, 0, 0, 0, 0);
  const U64 myB = offB[blockIdx.x] + mgBlockExclusive<TX_THREADS, MgSum> (nb, sScan);
  const U64 myQ = offQ[blockIdx.x] + mgBlockExclusive<TX_THREADS, MgSum> (nq, sScan);
  const U64 myE = offE[blockIdx.x] + mgBlockExclusive<TX_THREADS, MgSum> (ne, sScan) + 1;                     /* entry 0 is the accumulator's start */
  if (at >= n || (!nb && !ne)) return;
  if (myB + nb > basesCap || myE + ne > recCap) { *overflow = 1; return; }
  U32 x0 = 0, x1 = 0, x2 = 0, x3 = 0;
  tqWalk<true> (b, at, n, prev, line, textBase + at, &x0, &x1, &x2, &x3, bases, myB, myQ, endB, endQ, endP, myE);
}

/* Kq6: a record's sequence line and quality line are of one length (seqio.c:339), for the records completed in [first, last] */
__global__ void mgTextFastqCheckKernel (const U64 *__restrict__ endB, const U64 *__restrict__ endQ, U64 first, U64 last, TqState *st)
{
  const U64 r = first + (U64) blockIdx.x * blockDim.x + threadIdx.x;
  if (r > last) return;
  if (endB[r] - endB[r - 1] != endQ[r] - endQ[r - 1]) st->bad = 1;
}

/* ---------------------------------------------------------------------------------------- */
/* host side                                                                                  */

/* K1 for the other consumer of FASTA text (mg_internal.h) */
extern "C" int mgTextLaunchEventTiles (const unsigned char *dText, size_t n, U64 textBase, U32 prevByte, U64 *dTileEvent, void *stream)
{
  const U64 nTiles = (n + TX_TILE - 1) / TX_TILE;
  hipLaunchKernelGGL (mgTextEventKernel, dim3 ((unsigned) nTiles), dim3 (TX_THREADS), 0, (hipStream_t) stream, dText, (U64) n, textBase, prevByte, dTileEvent);
  return hipGetLastError () == hipSuccess ? 0 : -1;
}

/* one batch: records [0, nRec) of the accumulator, bases [0, total); dRecOff[nRec] == total.  Returns 0 or an error */
static int txFlush (TxBufs &t, const TxSink &sink, U64 total, U64 nRec, hipStream_t st, TxIds *ids)
{
  if (sink.wantIds && (ids->off.size () < nRec || (ids->off.size () == nRec && ids->open)))
    { mgSetError ("device text parser: %llu records but %llu ids", (unsigned long long) nRec, (unsigned long long) ids->off.size ()); return -1; }
  const size_t nw = mgPackedWords (total);
  if (t.dPacked.reserve (nw, nw + nw / 4, "device text parser")) return -1;
  if (mgLaunchPack (t.dBases.p, total, t.dPacked.p, st)) return -1;
  return sink.fn (sink.ctx, t.dPacked.p, total, t.dRecOff.p, (U32) nRec, sink.wantIds ? ids->bytes.data () : (const char *) 0, sink.wantIds ? ids->off.data () : (const U64 *) 0, st);
}

/* ---- what differs between the formats, for the one loop below.  Both keep the accumulator's counts as of the last synchronised window; every step
 * returns false where a HIP call failed ---- */
struct TxFormat {
  U64 accBases = 0, accRecs = 0, accQual = 0;
  bool bad = false;                                        /* FASTQ: a rule was broken in the accumulator's text */
  U64 resume = 0, resumeLine = 1;                          /* where the host parser would take over: FASTQ, the text offset behind the last record handed on; FASTA (a text of unknown size that ends in an unfinished record), the last record's '>' */
  bool sized = true;                                       /* the text's size was known before the walk, and so its last byte and its last line */
};
#define TX_GRID(nTiles, st) dim3 ((unsigned) (nTiles)), dim3 (TX_THREADS), 0, st      /* a workgroup a tile */
#define TX_ONE(st) dim3 (1), dim3 (MG_GROUP_THREADS), 0, st                          /* the one workgroup of a tile scan */
struct FaFormat : TxFormat {
  static constexpr bool fastq = false;
  U64 recsPrev = 0;                                        /* the accumulator's records before the current window */
  bool init (TxBufs &t)
  { TxState z; z.lastEvent = 0; z.accBases = 0; z.accRecs = 0;
    TqState q; memset (&q, 0, sizeof (q)); const U64 one = 1;      /* (a text of unknown size: the newlines so far in dTq, as FASTQ keeps them) */
    return hipMemcpy (t.dState.p, &z, sizeof (z), hipMemcpyHostToDevice) == hipSuccess
           && (sized || (hipMemcpy (t.dTq.p, &q, sizeof (q), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy (t.dOpenLine.p, &one, 8, hipMemcpyHostToDevice) == hipSuccess));
  }
  void count (TxBufs &t, const TxWalk &w, U64 nTiles, hipStream_t st)      /* K1 .. K4; a text of unknown size: Kq1 and Kq2 as well, the line number at every tile's first byte */
  { if (!sized)
      { hipLaunchKernelGGL (mgTextNewlineKernel, TX_GRID (nTiles, st), w.dText (), (U64) w.got.n, t.dTileOffQ.p);
        hipLaunchKernelGGL (mgTextLineScanKernel, TX_ONE (st), t.dTileOffQ.p, nTiles, t.dTq.p);
      }
    hipLaunchKernelGGL (mgTextEventKernel, TX_GRID (nTiles, st), w.dText (), (U64) w.got.n, w.off, w.prevByte, t.dTileEvent.p);
    hipLaunchKernelGGL (mgTextStateScanKernel, TX_ONE (st), t.dTileEvent.p, nTiles, t.dState.p);
    hipLaunchKernelGGL (mgTextCountKernel, TX_GRID (nTiles, st), w.dText (), (U64) w.got.n, w.off, w.prevByte, t.dTileEvent.p, t.dTileBases.p, t.dTileStarts.p);
    hipLaunchKernelGGL (mgTextOffsetScanKernel, TX_ONE (st), t.dTileBases.p, t.dTileStarts.p, nTiles, t.dTileBaseOff.p, t.dTileStartOff.p, t.dState.p, t.hCounts);
  }
  void counts (const U64 *h) { recsPrev = accRecs; accBases = h[0]; accRecs = h[1]; }
  void emit (TxBufs &t, const TxWalk &w, U64 nTiles, bool wantIds, hipStream_t st)
  { hipLaunchKernelGGL (mgTextEmitKernel, TX_GRID (nTiles, st), w.dText (), (U64) w.got.n, w.off, w.prevByte, t.dTileEvent.p, t.dTileBaseOff.p, t.dTileStartOff.p,
                        t.dBases.p, (U64) t.basesCap, t.dRecOff.p, (U64) t.recCap, t.dOverflow.p, wantIds || !sized ? t.dRecPos.p : (U64 *) 0);
    if (!sized && accRecs > recsPrev)                      /* a record starts in this window: the last of them is the open one now */
      hipLaunchKernelGGL (mgTextRecordLineKernel, dim3 (1), dim3 (TX_THREADS), 0, st, w.dText (), (U64) w.got.n, w.off, t.dRecPos.p, accRecs - 1, t.dTileOffQ.p, t.dOpenLine.p);
  }
  /* the records that start in this window: the id starts a byte after the '>' */
  bool headers (TxBufs &t, const TxWalk &, U64 recsBefore, TxHdrs *h) { h->dSrc = t.dRecPos.p + recsBefore; h->add = 1; h->n = (size_t) (accRecs - recsBefore); h->at0 = false; return true; }
  /* 0: go on; 1: the text ends here and its last record is unfinished -- the text's last byte is no newline, or its last line is a header (the two cases a
     sized text is declined for before the walk, mg_textgpu.hip; seqio.c:213-217,314): the records before the last are handed on, the host parser takes
     the last one up; -1.  The last line is a header if and only if the text's only newline from the last record's '>' on is its last byte; as before the
     walk, a header that does not lie within the text's last 4096 bytes is not judged */
  int verdict (TxBufs &t, const TxWalk &w, U64, hipStream_t st)
  { if (sized || !w.eof || !accRecs) return 0;
    TqState q; U64 line = 1, pos = 0;
    if (hipStreamSynchronize (st) != hipSuccess || hipMemcpy (&q, t.dTq.p, sizeof (q), hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy (&line, t.dOpenLine.p, 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (&pos, t.dRecPos.p + (accRecs - 1), 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const U64 end = w.off + w.got.n;
    const bool headerLast = w.got.last == '\n' && q.nlCount - (line - 1) == 1 && (end <= 4096 || end - pos < 4096);
    if (w.got.last == '\n' && !headerLast) return 0;
    resume = pos; resumeLine = line;
    return 1;
  }
  /* complete records: all of them at the end of the text, otherwise all but the one still open */
  bool cut (TxBufs &t, bool eof, U64 *nRec, U64 *total)
  { *nRec = eof ? accRecs : accRecs - 1; *total = accBases;
    return eof ? hipMemcpy (t.dRecOff.p + *nRec, total, 8, hipMemcpyHostToDevice) == hipSuccess : hipMemcpy (total, t.dRecOff.p + *nRec, 8, hipMemcpyDeviceToHost) == hipSuccess;
  }
  /* the open record's bases have moved to the front; it becomes record 0 of the next batch (lastEvent stays what it is on the device: only the two counters change) */
  bool flushed (TxBufs &t, bool eof, U64 total, hipStream_t st)
  { if (eof) return true;
    const U64 counters[2] = { accBases - total, 1 }, zero = 0;
    if (!sized && hipMemcpyAsync (t.dRecPos.p, t.dRecPos.p + (accRecs - 1), 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;      /* (where the open record's '>' is) */
    accBases = counters[0]; accRecs = 1;
    return hipMemcpyAsync ((char *) t.dState.p + offsetof (TxState, accBases), counters, 16, hipMemcpyHostToDevice, st) == hipSuccess
           && hipMemcpyAsync (t.dRecOff.p, &zero, 8, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize (st) == hipSuccess;
  }
};
struct FqFormat : TxFormat {
  static constexpr bool fastq = true;
  U64 nlCount = 0, tail[3] = { 0, 0, 0 };                  /* newlines of the text so far; bases, quality bytes, text position at the end of the last completed record */
  bool init (TxBufs &t)
  { TqState z; memset (&z, 0, sizeof (z)); const U64 zero = 0;
    return hipMemcpy (t.dTq.p, &z, sizeof (z), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy (t.dRecOff.p, &zero, 8, hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy (t.dEndQ.p, &zero, 8, hipMemcpyHostToDevice) == hipSuccess;
  }
  void count (TxBufs &t, const TxWalk &w, U64 nTiles, hipStream_t st)      /* Kq1 .. Kq4 */
  { hipLaunchKernelGGL (mgTextNewlineKernel, TX_GRID (nTiles, st), w.dText (), (U64) w.got.n, t.dTileEvent.p);
    hipLaunchKernelGGL (mgTextLineScanKernel, TX_ONE (st), t.dTileEvent.p, nTiles, t.dTq.p);
    hipLaunchKernelGGL (mgTextFastqCountKernel, TX_GRID (nTiles, st), w.dText (), (U64) w.got.n, w.prevByte, t.dTileEvent.p, t.dTileBases.p, t.dTileQual.p, t.dTileStarts.p, t.dTq.p);
    hipLaunchKernelGGL (mgTextFastqOffsetKernel, TX_ONE (st), t.dTileBases.p, t.dTileQual.p, t.dTileStarts.p, nTiles, t.dTileBaseOff.p, t.dTileOffQ.p, t.dTileStartOff.p, t.dTq.p, t.hCounts);
  }
  void counts (const U64 *h) { accBases = h[0]; accRecs = h[1]; accQual = h[2]; nlCount = h[3]; bad = h[4] != 0; }
  void emit (TxBufs &t, const TxWalk &w, U64 nTiles, bool, hipStream_t st)
  { hipLaunchKernelGGL (mgTextFastqEmitKernel, TX_GRID (nTiles, st), w.dText (), (U64) w.got.n, w.off, w.prevByte, t.dTileEvent.p, t.dTileBaseOff.p, t.dTileOffQ.p, t.dTileStartOff.p,
                        t.dBases.p, (U64) t.basesCap, t.dRecOff.p, t.dEndQ.p, t.dEndP.p, (U64) t.recCap, t.dOverflow.p);
  }
  /* a header starts at the text's first byte and after the last newline of every record this window completed -- but for the text's last record; the id
     starts a byte after the '@' */
  bool headers (TxBufs &t, const TxWalk &w, U64 recsBefore, TxHdrs *h)
  { h->dSrc = t.dEndP.p + recsBefore + 1; h->add = 2; h->n = (size_t) (accRecs - recsBefore); h->at0 = !w.off;
    if (h->n && w.eof)
      { U64 lastEnd = 0;
        if (hipMemcpy (&lastEnd, t.dEndP.p + accRecs, 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
        if (lastEnd + 1 >= w.off + w.got.n) --h->n;      /* (the text ends with this window: a source that inflates does not know where before) */
      }
    return true;
  }
  /* 0: go on; 1: nothing of the accumulator has been added, the host parser starts at its first record; -1 */
  int verdict (TxBufs &t, const TxWalk &w, U64 recsBefore, hipStream_t st)
  { const bool eof = w.eof;
    if (!bad && accRecs > recsBefore)                  /* the records this window completed: sequence and quality lines of one length? */
      { hipLaunchKernelGGL (mgTextFastqCheckKernel, dim3 ((unsigned) ((accRecs - recsBefore + 255) / 256)), dim3 (256), 0, st, t.dRecOff.p, t.dEndQ.p, recsBefore + 1, accRecs, t.dTq.p);
        TqState now;
        if (hipMemcpy (&now, t.dTq.p, sizeof (now), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        bad = now.bad != 0;
      }
    tail[0] = tail[1] = tail[2] = 0;
    if (accRecs && (hipMemcpy (&tail[0], t.dRecOff.p + accRecs, 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (&tail[1], t.dEndQ.p + accRecs, 8, hipMemcpyDeviceToHost) != hipSuccess
                    || hipMemcpy (&tail[2], t.dEndP.p + accRecs, 8, hipMemcpyDeviceToHost) != hipSuccess)) return -1;
    return bad || (eof && ((nlCount & 3) || accBases != tail[0] || accQual != tail[1])) ? 1 : 0;
  }
  bool cut (TxBufs &, bool, U64 *nRec, U64 *total) { *nRec = accRecs; *total = tail[0]; return true; }
  /* the open line's bases have moved to the front */
  bool flushed (TxBufs &t, bool eof, U64 total, hipStream_t st)
  { resume = tail[2] + 1;
    if (eof) return true;
    const U64 counters[3] = { accBases - total, accQual - tail[1], 0 };               /* accBases, accQual, accRecs */
    accBases = counters[0]; accQual = counters[1]; accRecs = 0;
    return hipMemcpyAsync ((char *) t.dTq.p + offsetof (TqState, accBases), counters, 24, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize (st) == hipSuccess;
  }
};

/* ---- the one parse loop.  Per window: the count kernels, the next window's load beside them, the counts, room for exactly what this window adds,
 * the emit kernel, the ids, the format's verdict, and a batch handed on where enough has come together ---- */
template <class F>
static int txParseLoop (const TxSrc &src, size_t textSize, bool sized, bool devIds, TxBufs &t, const TxSink &sink, U64 *nSeqOut, U64 *totLenOut, U64 *resumeOff, U64 *resumeLine)
{
  const size_t window = txWindowBytes (textSize);
  const U64 batch = txBatchBases (sink.batchBases), bigBatch = batch > txBatchBases (0) ? batch : txBatchBases (0);
  const int nThreads = txHostThreads ();
  const char *noRoom = "device text parser: allocation failed";
  hipStream_t st = 0;
  int rc = -1;
  U64 nSeq = 0, totLen = 0;
  F f; f.sized = sized;
  do {
    TxClock ck; ck.t0 = mgNowS ();
    if (txReserve (t, window, 1 << 20, 4096)) { mgSetError ("%s", noRoom); break; }      /* the accumulators grow to what the windows' counts ask for */
    ck.lap (ck.reserve);
    if (!f.init (t) || hipMemset (t.dOverflow.p, 0, 4) != hipSuccess) break;
    TxIds ids;
    TxWalk wk (t, src, window, st, &ck);
    if (wk.start ()) break;
    int end = wk.got.n ? -1 : 0;                           /* how the walk ends: -1 = a step failed (every plain break below), 0 = at the text's end, -3 = handed over */
    while (wk.got.n)
      { const U64 nTiles = (wk.got.n + TX_TILE - 1) / TX_TILE;
        ++gTxDiag[1]; gTxDiag[2] += wk.got.n;
        /* the window crosses the link and is counted, while the next one is loaded */
        if (wk.awaitCopy ()) break;
        f.count (t, wk, nTiles, st);
        if (hipGetLastError () != hipSuccess || wk.loadNext () || hipStreamSynchronize (st) != hipSuccess) break;
        const bool eof = wk.eof;
        const U64 recsBefore = f.accRecs;
        f.counts (t.hCounts);
        ck.lap (ck.wait);
        /* the counts are in: room for exactly what this window adds, then the bases and the offsets are written */
        if (f.accBases + 64 > t.basesCap || f.accRecs + 3 > t.recCap)
          if (txReserve (t, window, f.accBases + 64, f.accRecs + 3)) { mgSetError ("%s", noRoom); break; }
        f.emit (t, wk, nTiles, sink.wantIds, st);
        if (hipGetLastError () != hipSuccess) break;
        const bool wantIds = sink.wantIds && !f.bad;
        TxHdrs h;
        if ((wantIds && !f.headers (t, wk, recsBefore, &h)) || txHeadersOut (t, wantIds && !devIds, h, st)) break;
        if (wantIds)
          { ck.lap (ck.flush);
            if (txWindowIds (t, ids, devIds, wk, h, nThreads, st)) break;
            ck.lap (ck.ids);
          }
        U32 ov = 0; if (hipMemcpy (&ov, t.dOverflow.p, 4, hipMemcpyDeviceToHost) != hipSuccess || ov) { mgSetError ("device text parser: accumulator overflow"); break; }
        const int v = f.verdict (t, wk, recsBefore, st);
        if (v < 0 || (v && F::fastq)) { if (v > 0) end = -3; break; }      /* FASTQ: nothing of the accumulator is handed on */
        if (eof || f.accBases >= bigBatch || (f.accBases >= batch && f.accRecs >= sink.batchRecs))
          { U64 nRec = 0, total = 0;
            if (!f.cut (t, eof && !v, &nRec, &total)) break;      /* (FASTA that ends in an unfinished record: all but that one, as in mid-text) */
            if (nRec)
              { ck.lap (ck.flush);
                if (txFlush (t, sink, total, nRec, st, &ids)) break;
                ck.lap (ck.sink);
                nSeq += nRec; totLen += total;
                if (sink.wantIds) ids.dropFront ((size_t) nRec);
                if (!eof) txCarry (t.dBases.p, total, f.accBases - total, st);      /* what is not handed on moves to the front */
                if (!f.flushed (t, eof, total, st)) break;
              }
          }
        if (v) { end = -3; break; }
        wk.advance ();
        if (!wk.got.n) end = 0;
      }
    ck.lap (ck.flush);
    if (txTiming () && F::fastq) fprintf (stderr, "  [device text] FASTQ: reserve %.3f s, read %.3f, wait for the device %.3f, record ids %.3f, pack + sink %.3f, emit + rest %.3f\n", ck.reserve, ck.read, ck.wait, ck.ids, ck.sink, ck.flush);
    if (txTiming () && !F::fastq) fprintf (stderr, "  [device text] FASTA: reserve %.3f s, read %.3f, wait for the device %.3f, emit + flush + rest %.3f\n", ck.reserve, ck.read, ck.wait, ck.flush + ck.ids + ck.sink);
    if (txTiming () && (F::fastq || sink.wantIds)) fprintf (stderr, "  [device text] ids: the team's two passes %.3f (%d threads), the id kernels %.3f\n", ids.tLens, nThreads, ids.tDev);
    if (end == -1)
      { wk.drain ();
        if (!mgLastError ()[0]) mgSetError ("device text parser: HIP failure (%s)", hipGetErrorString (hipGetLastError ()));
        break;
      }
    rc = end;
  } while (0);
  if (nSeqOut) *nSeqOut = nSeq;
  if (totLenOut) *totLenOut = totLen;
  if (resumeOff) *resumeOff = f.resume;
  if (resumeLine) *resumeLine = F::fastq ? 4 * nSeq + 1 : f.resumeLine;
  if (rc == -3) gTxDiag[3] = f.resume;
  return rc;
}
int txParseText (bool fastq, const TxSrc &src, size_t textSize, bool sized, bool devIds, TxBufs &t, const TxSink &sink, U64 *nSeqOut, U64 *totLenOut, U64 *resumeOff, U64 *resumeLine)
{
  return fastq ? txParseLoop<FqFormat> (src, textSize, sized, devIds, t, sink, nSeqOut, totLenOut, resumeOff, resumeLine)
               : txParseLoop<FaFormat> (src, textSize, sized, devIds, t, sink, nSeqOut, totLenOut, resumeOff, resumeLine);
}
