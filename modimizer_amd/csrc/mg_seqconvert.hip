/* mg_seqconvert.hip — the reference's `seqconvert -fa|-fq` (seqconvert.c over seqIOread / seqIOwrite, seqio.c:234-346,463-545) and `seqhoco`
 * (seqhoco.c) on the device: a FASTA or FASTQ file rewritten as FASTA or FASTQ, optionally homopolymer-compressed.  Every byte is classified,
 * compacted and re-emitted here; the host reads, inflates, deflates and writes.
 *
 * The text goes through the device text parser's window loop (mgTextStreamWindows) in tiles of 4 KiB, 16 bytes a thread (txLoad).  What a byte
 * is depends on a small state -- outside a header / in the id / behind the id's separator / in the description -- that every byte maps onto
 * itself: a record start sets it, a newline sets it, white space moves id -> separator -> description.  Such maps compose associatively, so
 * the state at every byte is a prefix scan over 8-bit maps (four states, two bits each; sqThen); the FASTQ line of a byte is a prefix sum
 * of newlines (txNewlines).  Per window:
 *
 *   F  per tile: the composition of its bytes' maps, its newlines;
 *   S  one workgroup: the state and the line at every tile's first byte, on top of what the window before ended in;
 *   M  per tile, measure: every byte's role and what it adds to the output; the running counts of id, description, sequence and quality bytes
 *      (four 16-bit fields of one word inside a tile) and their values at the record boundaries -- FASTA: a '>' that begins a line ends the
 *      record before it; FASTQ: the fourth newline.  A record's id, description and sequence lengths are the differences of the counts
 *      between two boundaries; the counts only grow, so "the counts at the last boundary" is a running maximum (as mg_composition.hip's);
 *   X  one workgroup: the counts and the last boundary across the tiles (and windows), the records that end at a tile's first boundary,
 *      the last kept base before every tile (MG_SEQ_HOCO), and the exclusive sum of the tiles' output bytes;
 *   W  per tile, write: the same walk once more, every byte to its place in the window's output buffer.
 *
 * FASTA -> FASTQ writes '!' for every base behind a record's last base: the output buffer is preset to '!' (one memset a window) and W steps
 * over the run; the part of a run that belongs to bases of EARLIER windows (one run a window at most) is not in the buffer: the writer
 * thread splices that many '!' in at the place W reports, so the buffer is bounded by the window (sqOutCap: a record without a sequence line
 * GROWS -- ">\n" becomes ">\n\n", or "@\n\n+\n\n" -- so the bound is 1.5 n and 3 n for FASTA in) and a 125 Mbp record costs its bytes.  MG_SEQ_HOCO writes a kept base iff it differs from the kept base before it in the
 * same record: that base is a running maximum of (position, base) codes, valid if it lies behind the last boundary; inside M a tile does not
 * know it yet and counts its first kept base as written, X takes that back where the base before the tile says so.
 *
 * The text goes through twice.  The first walk (F S M X) judges it: what the programs die () on, bytes they would index a table out of bounds
 * with, where the last complete record ends, where seqhoco stops (its first record without a base; the record's header would already be
 * written when a single walk found out).  Nothing is written before that is known; the second walk (F S M X W) sees only the text that is
 * written, which ends in a complete record.  Window i's output is copied out on a stream of its own while window i + 1 is in the kernels, and
 * written by a thread of its own. */
#include "mg_prefix.h"
#include "mg_internal.h"
#include "mg_textsrc.h"
#include "mg_textsink.h"

#define SQ_THREADS 256
#define SQ_WAVES   (SQ_THREADS / 64)
#define SQ_TILE    (SQ_THREADS * 16)
static_assert (SQ_TILE == MG_TEXT_TILE, "the parser's tile");
#define SQ_NONE    (~(U64) 0)
#define SQ_MAXLEN  ((U64) 1 << 31)                      /* the reference's lengths are int */

/* the header state and the maps over it: map f sends state s to (f >> 2 s) & 3 */
enum { SQ_NOTHDR = 0, SQ_ID = 1, SQ_SEP = 2, SQ_DESC = 3 };
#define SQ_FN_IDENT 0xe4u
#define SQ_FN_SPACE 0xf8u                                 /* id -> separator -> description */
#define SQ_FN_OTHER 0xf4u                                 /* separator -> description */
#define SQ_FN_TO(s) (0x55u * (s))

__device__ __forceinline__ bool sqIsSpace (U32 c) { return c == ' ' || (c >= 9 && c <= 13); }      /* isspace in the C locale */
__device__ __forceinline__ U32 sqFnOf (U32 c, U32 prev, int fastq)
{
  const U64 e = txEvent (c, prev, 0);                    /* the parser's rule: newline -> even, '>' behind a newline -> odd */
  if (e) return (e & 1) ? (fastq ? SQ_FN_OTHER : SQ_FN_TO (SQ_ID)) : SQ_FN_TO (fastq ? SQ_ID : SQ_NOTHDR);
  return sqIsSpace (c) ? SQ_FN_SPACE : SQ_FN_OTHER;
}
__device__ __forceinline__ U32 sqThen (U32 a, U32 b)      /* a, then b */
{
  U32 r = 0;
#pragma unroll
  for (int s = 0 ; s < 4 ; ++s) r |= ((b >> (2 * ((a >> (2 * s)) & 3u))) & 3u) << (2 * s);
  return r;
}
__device__ __forceinline__ U32 sqApply (U32 f, U32 s) { return (f >> (2 * s)) & 3u; }

/* thread t gets f(0) then ... then f(t - 1) (the identity for thread 0), *total the workgroup's; not mg_prefix.h's: the order matters.  lds: SQ_WAVES words */
__device__ __forceinline__ U32 sqBlockExclusiveFn (U32 f, U32 *lds, U32 *total)
{
  const U32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  U32 inc = f;
  for (int off = 1 ; off < 64 ; off <<= 1) { const U32 o = mgLaneUp (inc, off); if (lane >= (U32) off) inc = sqThen (o, inc); }
  if (lane == 63u) lds[wv] = inc;
  __syncthreads ();
  U32 before = SQ_FN_IDENT, tot = SQ_FN_IDENT;
#pragma unroll
  for (U32 i = 0 ; i < SQ_WAVES ; ++i) { const U32 s = lds[i]; if (i < wv) before = sqThen (before, s); tot = sqThen (tot, s); }
  __syncthreads ();
  const U32 up = mgLaneUp (inc, 1);
  *total = tot;
  return sqThen (before, lane ? up : SQ_FN_IDENT);
}

__device__ __forceinline__ void sqMax64 (U64 *p, U64 v) { atomicMax ((unsigned long long *) p, (unsigned long long) v); }
__device__ __forceinline__ void sqMin64 (U64 *p, U64 v) { atomicMin ((unsigned long long *) p, (unsigned long long) v); }
__device__ __forceinline__ void sqAdd64 (U64 *p, U64 v) { atomicAdd ((unsigned long long *) p, (unsigned long long) v); }

/* dna2textAmbigConv (seqio.c:621-630): ABCDGHKMNRSTVWY in either case -> the upper-case letter, '-' stays, else 0; dna2textConv: ACGTNacgtn stay */
#define SQ_AMBIG 0x2dc699eu
#define SQ_ACGTN 0x0010408au
__device__ __forceinline__ U32 sqKeepAmbig (U32 c) { if (c == '-') return c; return ((c & 0xc0u) == 0x40u && ((SQ_AMBIG >> (c & 0x1fu)) & 1u)) ? (c & 0xdfu) : 0u; }
__device__ __forceinline__ U32 sqKeepAcgtn (U32 c) { return ((c & 0xc0u) == 0x40u && ((SQ_ACGTN >> (c & 0x1fu)) & 1u)) ? c : 0u; }

struct SqCfg { int fastq, outFastq, hoco, written; };     /* written: sequence bytes count as they are written (the second walk), else as the input filter keeps them */

enum { SQ_I = 0, SQ_D, SQ_K, SQ_Q };                      /* the four running counts: id, description, sequence, quality bytes */
__device__ __forceinline__ U64 sqField (U64 packed, int c) { return (packed >> (16 * c)) & 0xffffu; }

struct SqState {                                           /* device resident, carried from window to window; read back once */
  U64 hstate, line;              /* the header state behind the text so far; its newlines */
  U64 V[4], VB[4];               /* the running counts; their values at the last boundary */
  U64 bSeen, Bpos;               /* a boundary so far; position + 1 of the last one */
  U64 lastKept;                  /* MG_SEQ_HOCO, FASTA: ((position + 1) << 8) | upper case of the last base the filter kept */
  U64 nRec, maxSeq, maxId, maxDesc, totFilt;
  U64 errLine, errOff;           /* FASTQ: the first line that breaks a rule (line mod 4 says which), the offset it is seen at; SQ_NONE */
  U64 badOff, nulOff, badLine;   /* the first byte the reference indexes a table out of bounds with / NUL in a header line; the line of the earlier one */
  U64 stopStart, stopEnd;        /* the first record without a sequence byte: where it starts, the byte behind it; SQ_NONE */
  U64 hdrEnd, tooLong, crossed;
};
struct SqWin { U64 outBytes, spliceAt, spliceCount, spliceTile; };      /* a window's output: its bytes; spliceCount '!' belong in front of byte spliceAt */

struct SqTiles {                                           /* per tile of the window */
  U32 *fn, *nl, *state; U64 *line;                         /* F, S */
  U32 *cnt[4]; U64 *off[4];                                /* M: the tile's four counts; X: their exclusive sums */
  U64 *lastCode, *firstV;                                  /* M: the packed counts (tile relative) at the tile's last boundary, + 1 (0: none) / at its first */
  U64 *lastB, *firstB, *firstLine;                         /* M: position + 1 of the last / the first boundary (0: none), line of the first */
  U32 *out, *firstFill; U64 *outSum, *outOff;              /* M: output bytes; X: the '!' run of the first boundary, the sums */
  U64 *lastKept, *keptIn; U32 *firstKept;                  /* MG_SEQ_HOCO, FASTA */
  U64 *prevTile;
};
#define SQ_TILE_ARRAYS 25

/* ---- the walk over a thread's 16 bytes ---- */

struct SqLane {
  U32 s; U64 line; U32 pk;           /* the header state, the line, the kept base before (upper case, 0: none in this record) */
  U64 v; U32 nb; U64 vAtLast, lastB; /* packed counts of the thread so far; its boundaries, the counts at and position + 1 of the last */
  U32 filt; U64 lastKept; U32 firstThing;      /* bytes the filter kept; the last one's code; what the thread meets first: 1 a boundary, 2 | base << 8 a kept base */
  __device__ __forceinline__ void init (U32 s_, U64 line_, U32 pk_) { s = s_; line = line_; pk = pk_; v = 0; nb = 0; vAtLast = 0; lastB = 0; filt = 0; lastKept = 0; firstThing = 0; }
};

/* what a walk does with the roles: nothing */
struct SqHookNone {
  __device__ __forceinline__ U32 boundary (const SqLane &, U64, U64, bool) { return 0; }
  __device__ __forceinline__ void put (U32) {}
  __device__ __forceinline__ void skip (U32) {}
  __device__ __forceinline__ void rule (U64, U64) {}
  __device__ __forceinline__ void bad (U64, U64, bool) {}
  __device__ __forceinline__ void hdrEnd (U64) {}
};

template <class H> __device__ __forceinline__ void sqKept (const SqCfg &g, SqLane &t, H &h, U32 u, U64 pos)
{
  const U32 up = u & 0xdfu;
  ++t.filt; t.lastKept = ((pos + 1) << 8) | up;
  if (!t.firstThing) t.firstThing = 2u | (up << 8);
  bool w = true;
  if (g.hoco && g.written) { w = up != t.pk; t.pk = up; }
  if (w) { t.v += (U64) 1 << (16 * SQ_K); h.put (u); }
}

template <class H> __device__ __forceinline__ void sqHeader (const SqCfg &g, SqLane &t, H &h, U32 c, U64 pos)
{
  if (c == '\n')
    { h.put ('\n');
      if (g.fastq) ++t.line; else h.hdrEnd (pos + 1);
      t.s = g.fastq ? SQ_ID : SQ_NOTHDR; t.pk = 0;
      return;
    }
  if (!c) h.bad (pos, t.line + 1, true);                   /* the program's strlen would end the name here */
  if (t.s == SQ_ID) { if (sqIsSpace (c)) t.s = SQ_SEP; else { t.v += 1; h.put (c); } }
  else
    { const bool first = t.s == SQ_SEP;
      t.s = SQ_DESC;
      if (!g.hoco) { t.v += (U64) 1 << (16 * SQ_D); if (first) h.put (' '); h.put (c); }      /* seqhoco passes no description (seqhoco.c:31) */
    }
}

template <class H> __device__ __forceinline__ void sqBoundary (SqLane &t, H &h, U64 pos)
{
  ++t.nb; t.vAtLast = t.v; t.lastB = pos + 1; t.pk = 0;
  if (!t.firstThing) t.firstThing = 1;
}

template <class H> __device__ __forceinline__ void sqRun (const SqCfg &g, const unsigned char *b, U32 prev0, U64 at, U64 n, U64 textBase, SqLane &t, H &h)
{
  U32 prev = prev0;
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j)
    { if (at + j < n)
        { const U32 c = b[j];
          const U64 pos = textBase + at + j;
          if (!g.fastq)
            { if (c == '>' && prev == '\n')                /* ends the record before it (there is one unless this is the text's first byte), starts the next */
                { const bool open = pos != 0;
                  const U32 fill = h.boundary (t, pos, t.line, open);
                  if (open) { h.put ('\n'); if (g.outFastq) { h.put ('+'); h.put ('\n'); h.skip (fill); h.put ('\n'); } }
                  h.put (g.outFastq ? '@' : '>');
                  sqBoundary (t, h, pos);
                  t.s = SQ_ID;
                }
              else if (t.s == SQ_NOTHDR)
                { if (c == '\n') ++t.line;
                  else if (c >= 0x80u) h.bad (pos, 0, false);      /* convert[] has 128 entries (seqio.c:322) */
                  else { const U32 u = g.hoco ? sqKeepAcgtn (c) : sqKeepAmbig (c); if (u) sqKept (g, t, h, u, pos); }
                }
              else { if (c == '\n') ++t.line; sqHeader (g, t, h, c, pos); }
            }
          else
            { const U32 phase = (U32) t.line & 3u;
              if (phase == 0)
                { if (prev == '\n')
                    { if (c != '@') h.rule (t.line + 1, pos);      /* seqio.c:302 */
                      if (c == '\n') ++t.line; else h.put (g.outFastq ? '@' : '>');
                      t.s = SQ_ID;
                    }
                  else sqHeader (g, t, h, c, pos);
                }
              else if (phase == 1)
                { if (prev == '\n') t.pk = 0;
                  if (c == '\n') { h.put ('\n'); ++t.line; }
                  else if (g.hoco && !sqKeepAcgtn (c)) { ++t.filt; t.v += (U64) 1 << (16 * SQ_K); h.bad (pos, t.line + 1, false); }      /* seqhoco converts it to -2 and indexes with that; it is a byte of the line all the same (seqio.c:338) */
                  else sqKept (g, t, h, c, pos);
                }
              else if (phase == 2)
                { if (prev == '\n' && c != '+') h.rule (t.line + 1, pos);      /* seqio.c:333 */
                  if (c == '\n') { if (g.outFastq) h.put ('\n'); ++t.line; }
                  else if (prev == '\n' && g.outFastq) h.put ('+');
                }
              else if (c == '\n')
                { (void) h.boundary (t, pos, t.line, true);
                  if (g.outFastq) h.put ('\n');
                  sqBoundary (t, h, pos);
                  ++t.line;
                }
              else { t.v += (U64) 1 << (16 * SQ_Q); if (g.outFastq) h.put (c); }
            }
        }
      prev = b[j];
    }
}

/* the first walk of M and W: counts, and what ends the file early */
struct SqHookCount {
  U32 nOut = 0; U64 errLine = SQ_NONE, errOff = SQ_NONE, badOff = SQ_NONE, nulOff = SQ_NONE, badLine = SQ_NONE, hdr = 0;
  __device__ __forceinline__ U32 boundary (const SqLane &, U64, U64, bool) { return 0; }
  __device__ __forceinline__ void put (U32) { ++nOut; }
  __device__ __forceinline__ void skip (U32) {}
  __device__ __forceinline__ void rule (U64 line1, U64 pos) { if (errLine == SQ_NONE) { errLine = line1; errOff = pos; } }
  __device__ __forceinline__ void bad (U64 pos, U64 line1, bool nul)
  { if (badLine == SQ_NONE) badLine = line1;
    if (nul) { if (nulOff == SQ_NONE) nulOff = pos; } else if (badOff == SQ_NONE) badOff = pos;
  }
  __device__ __forceinline__ void hdrEnd (U64 p) { hdr = p; }
};

/* the second walk: the records that end inside the tile, and the '!' runs they add.  KIND 0: M (the records are judged and counted), 1: W's
   count of the output bytes, 2: W's writes */
template <int KIND> struct SqHookRecords {
  const SqCfg &g; const SqTiles &T; SqState *st; SqWin *win; U64 tile;
  U64 vMine, prevCode, bPrev;
  U32 nOut = 0; U64 maxSeq = 0, maxId = 0, maxDesc = 0;
  unsigned char *dst = 0; U64 cur = 0, cap = 0; bool markSplice = false;
  __device__ __forceinline__ SqHookRecords (const SqCfg &g_, const SqTiles &T_, SqState *st_, SqWin *win_, U64 tile_, U64 vMine_, U64 prevCode_, U64 bPrev_)
    : g (g_), T (T_), st (st_), win (win_), tile (tile_), vMine (vMine_), prevCode (prevCode_), bPrev (bPrev_) {}
  __device__ __forceinline__ U32 boundary (const SqLane &t, U64 pos, U64 line, bool open)
  { const bool fillMode = !g.fastq && g.outFastq;
    const U64 vNow = vMine + t.v;
    U64 prevV, startB;
    if (t.nb) { prevV = vMine + t.vAtLast; startB = t.lastB; }
    else if (prevCode) { prevV = prevCode - 1; startB = bPrev; }
    else                                                  /* the tile's first boundary: the record began in an earlier tile, X has its length */
      { if (KIND == 0) { T.firstV[tile] = vNow; T.firstB[tile] = pos + 1; T.firstLine[tile] = line; return 0; }
        if (KIND == 2 && tile == win->spliceTile) markSplice = true;
        return fillMode ? T.firstFill[tile] : 0;
      }
    const U64 d = vNow - prevV;                           /* every field grows: no borrow */
    const U32 k = (U32) sqField (d, SQ_K);
    if (KIND == 0)
      { if (k > maxSeq) maxSeq = k;
        if (sqField (d, SQ_I) > maxId) maxId = sqField (d, SQ_I);
        if (sqField (d, SQ_D) > maxDesc) maxDesc = sqField (d, SQ_D);
        if (g.fastq && !g.written && k != (U32) sqField (d, SQ_Q)) { sqMin64 (&st->errLine, line + 1); sqMin64 (&st->errOff, pos); }      /* seqio.c:338 */
        if (!k) { sqMin64 (&st->stopStart, g.fastq ? startB : startB - 1); sqMin64 (&st->stopEnd, g.fastq ? pos + 1 : pos); }
      }
    (void) open;
    return fillMode ? k : 0;
  }
  __device__ __forceinline__ void put (U32 c) { if (KIND == 2) { if (cur < cap) dst[cur] = (unsigned char) c; ++cur; } else ++nOut; }
  __device__ __forceinline__ void skip (U32 n)
  { if (KIND == 2) { if (markSplice) { win->spliceAt = cur; markSplice = false; } cur += n; } else nOut += n; }
  __device__ __forceinline__ void rule (U64, U64) {}
  __device__ __forceinline__ void bad (U64, U64, bool) {}
  __device__ __forceinline__ void hdrEnd (U64) {}
};

/* ======================================================================================== */

/* F */
__global__ __launch_bounds__ (SQ_THREADS)
void mgSeqFnKernel (const unsigned char *__restrict__ text, U64 n, U32 prevByte, int fastq, U32 *__restrict__ tileFn, U32 *__restrict__ tileNl)
{
  __shared__ U32 s32[SQ_WAVES];
  const U64 at = ((U64) blockIdx.x * SQ_THREADS + threadIdx.x) * 16;
  U32 f = SQ_FN_IDENT, nl = 0;
  if (at < n)
    { unsigned char b[16]; U32 prev;
      txLoad (text, n, at, prevByte, b, &prev);
      nl = txNewlines (b, at, n);
#pragma unroll
      for (int j = 0 ; j < 16 ; ++j) { if (at + j < n) f = sqThen (f, sqFnOf (b[j], prev, fastq)); prev = b[j]; }
    }
  U32 total;
  (void) sqBlockExclusiveFn (f, s32, &total);
  nl = mgBlockReduce<SQ_THREADS, MgSum> (nl, s32);
  if (threadIdx.x == 0) { tileFn[blockIdx.x] = total; tileNl[blockIdx.x] = nl; }
}

/* S: edge: 0 the text's first window, 1 the window begins with a record, 2 it does not as far as the host can tell (FASTQ: the line says) */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgSeqStateScanKernel (SqTiles T, U64 nTiles, int fastq, int edge, SqState *st)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  U32 *lf = (U32 *) lds;
  const U32 tid = threadIdx.x;
  const U64 per = (nTiles + (MG_GROUP_THREADS - 1)) / MG_GROUP_THREADS;
  const U64 lo = (U64) tid * per < nTiles ? (U64) tid * per : nTiles, hi = lo + per < nTiles ? lo + per : nTiles;
  const U32 carry = fastq && !edge ? SQ_ID : (U32) st->hstate;      /* FASTQ text begins as a line does: behind a newline */
  const U64 lineIn = st->line;
  U32 acc = SQ_FN_IDENT;
  for (U64 i = lo ; i < hi ; ++i) acc = sqThen (acc, T.fn[i]);
  lf[tid] = acc;
  __syncthreads ();
  for (U32 off = 1 ; off < MG_GROUP_THREADS ; off <<= 1)
    { const U32 o = tid >= off ? lf[tid - off] : SQ_FN_IDENT;
      __syncthreads ();
      lf[tid] = sqThen (o, lf[tid]);
      __syncthreads ();
    }
  U32 run = tid ? lf[tid - 1] : SQ_FN_IDENT;
  const U32 all = lf[MG_GROUP_THREADS - 1];
  __syncthreads ();
  for (U64 i = lo ; i < hi ; ++i) { T.state[i] = sqApply (run, carry); run = sqThen (run, T.fn[i]); }
  const U64 line = mgGroupScan<MgSum> (T.nl, T.line, nTiles, lineIn, lds);
  if (tid == 0)
    { if (edge == 2 || (fastq && edge == 1 && (lineIn & 3u))) ++st->crossed;
      st->hstate = sqApply (all, carry); st->line = line;
    }
}

/* M (WRITE 0) and W (WRITE 1) */
template <int WRITE> __global__ __launch_bounds__ (SQ_THREADS)
void mgSeqTileKernel (const unsigned char *__restrict__ text, U64 n, U64 textBase, U32 prevByte, SqCfg g, SqTiles T, unsigned char *out, U64 outCap, SqWin *win, SqState *st)
{
  __shared__ U64 s64[SQ_WAVES];
  __shared__ U32 s32[SQ_WAVES];
  const U64 tile = blockIdx.x;
  const U64 at = (tile * SQ_THREADS + threadIdx.x) * 16;
  unsigned char b[16]; U32 prev0 = 0, f = SQ_FN_IDENT, nl = 0;
  const bool live = at < n;
  if (live)
    { txLoad (text, n, at, prevByte, b, &prev0);
      nl = txNewlines (b, at, n);
      U32 prev = prev0;
#pragma unroll
      for (int j = 0 ; j < 16 ; ++j) { if (at + j < n) f = sqThen (f, sqFnOf (b[j], prev, g.fastq)); prev = b[j]; }
    }
  U32 ftot, nltot;
  const U32 state = sqApply (sqBlockExclusiveFn (f, s32, &ftot), T.state[tile]);
  const U64 line = T.line[tile] + (mgBlockInclusive<SQ_THREADS, MgSum> (nl, s32, &nltot) - nl);
  /* MG_SEQ_HOCO: the kept base before the thread's first byte */
  U32 pk = 0;
  if (g.hoco && g.written)
    { if (g.fastq) pk = ((U32) line & 3u) == 1u && prev0 != '\n' ? (prev0 & 0xdfu) : 0u;      /* the sequence is one line of nothing but bases */
      else
        { SqLane k; k.init (state, line, 0);
          SqHookNone none;
          if (live) sqRun (g, b, prev0, at, n, textBase, k, none);
          const U64 keptEx = mgBlockExclusive<SQ_THREADS, MgMax> (k.lastKept, s64), bEx = mgBlockExclusive<SQ_THREADS, MgMax> (k.lastB, s64);
          if (keptEx) pk = (keptEx >> 8) > bEx ? (U32) (keptEx & 0xffu) : 0u;
          else if (!bEx) pk = WRITE ? (U32) T.keptIn[tile] : 0u;      /* M: not known yet, the tile's first kept base counts as written until X says otherwise */
          if (!WRITE)
            { const U64 lastKept = mgBlockReduce<SQ_THREADS, MgMax> (k.lastKept, s64);
              const U32 first = mgBlockReduce<SQ_THREADS, MgMax> (k.firstThing ? ((SQ_THREADS - threadIdx.x) << 16) | k.firstThing : 0u, s32);      /* the lowest thread that met anything */
              if (threadIdx.x == 0) { T.lastKept[tile] = lastKept; T.firstKept[tile] = (first & 0xffu) == 2u ? (first >> 8) & 0xffu : 0u; }
            }
        }
    }
  /* the thread's counts and boundaries */
  SqLane a; a.init (state, line, pk);
  SqHookCount hc;
  if (live) sqRun (g, b, prev0, at, n, textBase, a, hc);
  U64 tileV;
  const U64 vMine = mgBlockInclusive<SQ_THREADS, MgSum> (a.v, s64, &tileV) - a.v;
  const U64 code = a.nb ? vMine + a.vAtLast + 1 : 0;
  const U64 prevCode = mgBlockExclusive<SQ_THREADS, MgMax> (code, s64), lastCode = mgBlockReduce<SQ_THREADS, MgMax> (code, s64);
  const U64 bPrev = mgBlockExclusive<SQ_THREADS, MgMax> (a.lastB, s64);
  if (!WRITE)
    { const U64 bLast = mgBlockReduce<SQ_THREADS, MgMax> (a.lastB, s64);
      if (hc.errLine != SQ_NONE) { sqMin64 (&st->errLine, hc.errLine); sqMin64 (&st->errOff, hc.errOff); }
      if (hc.badOff != SQ_NONE) sqMin64 (&st->badOff, hc.badOff);
      if (hc.nulOff != SQ_NONE) sqMin64 (&st->nulOff, hc.nulOff);
      if (hc.badLine != SQ_NONE) sqMin64 (&st->badLine, hc.badLine);
      if (hc.hdr) sqMax64 (&st->hdrEnd, hc.hdr);
      SqLane r; r.init (state, line, pk);
      SqHookRecords<0> hr (g, T, st, win, tile, vMine, prevCode, bPrev);
      if (live) sqRun (g, b, prev0, at, n, textBase, r, hr);
      const U32 tileOut = mgBlockReduce<SQ_THREADS, MgSum> (hr.nOut, s32);
      const U32 nb = mgBlockReduce<SQ_THREADS, MgSum> (a.nb, s32), filt = mgBlockReduce<SQ_THREADS, MgSum> (a.filt, s32);
      const U64 maxSeq = mgBlockReduce<SQ_THREADS, MgMax> (hr.maxSeq, s64), maxId = mgBlockReduce<SQ_THREADS, MgMax> (hr.maxId, s64), maxDesc = mgBlockReduce<SQ_THREADS, MgMax> (hr.maxDesc, s64);
      if (threadIdx.x == 0)
        { for (int c = 0 ; c < 4 ; ++c) T.cnt[c][tile] = (U32) sqField (tileV, c);
          T.lastCode[tile] = lastCode; T.lastB[tile] = bLast; T.out[tile] = tileOut;
          if (nb) sqAdd64 (&st->nRec, nb);
          if (filt) sqAdd64 (&st->totFilt, filt);
          if (maxSeq) sqMax64 (&st->maxSeq, maxSeq);
          if (maxId) sqMax64 (&st->maxId, maxId);
          if (maxDesc) sqMax64 (&st->maxDesc, maxDesc);
        }
    }
  else
    { U32 mine = hc.nOut;
      if (!g.fastq && g.outFastq)                           /* the '!' runs count */
        { SqLane r; r.init (state, line, pk);
          SqHookRecords<1> hr (g, T, st, win, tile, vMine, prevCode, bPrev);
          if (live) sqRun (g, b, prev0, at, n, textBase, r, hr);
          mine = hr.nOut;
        }
      U32 tileOut;
      const U32 before = mgBlockInclusive<SQ_THREADS, MgSum> (mine, s32, &tileOut) - mine;
      SqLane w; w.init (state, line, pk);
      SqHookRecords<2> hw (g, T, st, win, tile, vMine, prevCode, bPrev);
      hw.dst = out; hw.cur = T.outOff[tile] + before; hw.cap = outCap;
      if (live) sqRun (g, b, prev0, at, n, textBase, w, hw);
    }
}

/* X */
__global__ __launch_bounds__ (MG_GROUP_THREADS)
void mgSeqStitchKernel (SqTiles T, U64 nTiles, SqCfg g, SqWin *win, SqState *st)
{
  __shared__ U64 lds[MG_GROUP_THREADS];
  const U32 tid = threadIdx.x;
  const bool fillMode = !g.fastq && g.outFastq;
  if (tid == 0) { win->outBytes = 0; win->spliceAt = 0; win->spliceCount = 0; win->spliceTile = SQ_NONE; }
  U64 keptAll = 0;
  if (g.hoco && g.written && !g.fastq)                     /* the kept base in front of every tile; a tile whose first kept base repeats it wrote one byte too many */
    { keptAll = mgGroupScan<MgMax> (T.lastKept, T.keptIn, nTiles, st->lastKept, lds);
      (void) mgGroupScan<MgMax> (T.lastB, T.prevTile, nTiles, st->Bpos, lds);
      __syncthreads ();
      for (U64 t = tid ; t < nTiles ; t += MG_GROUP_THREADS)
        { const U64 code = T.keptIn[t];
          const U32 up = code && (code >> 8) > T.prevTile[t] ? (U32) (code & 0xffu) : 0u;
          T.keptIn[t] = up;
          if (up && T.firstKept[t] == up)
            { T.cnt[SQ_K][t] -= 1; T.out[t] -= 1;
              if (T.lastCode[t]) { T.lastCode[t] -= (U64) 1 << (16 * SQ_K); T.firstV[t] -= (U64) 1 << (16 * SQ_K); }
            }
        }
      __syncthreads ();
    }
  U64 tot[4];
  for (int c = 0 ; c < 4 ; ++c) { tot[c] = mgGroupScan<MgSum> (T.cnt[c], T.off[c], nTiles, st->V[c], lds); __syncthreads (); }
  for (U64 t = tid ; t < nTiles ; t += MG_GROUP_THREADS) T.prevTile[t] = T.lastCode[t] ? t + 1 : 0;
  __syncthreads ();
  const U64 lastTile = mgGroupScan<MgMax> (T.prevTile, T.prevTile, nTiles, (U64) 0, lds);      /* [t]: the last tile before t with a boundary, + 1 */
  __syncthreads ();
  U64 maxSeq = 0, maxId = 0, maxDesc = 0;
  for (U64 t = tid ; t < nTiles ; t += MG_GROUP_THREADS)
    { U32 fill = 0;
      if (T.lastCode[t])                                   /* the record that ends at the tile's first boundary */
        { const U64 p = T.prevTile[t];
          const bool open = g.fastq || p || st->bSeen;
          if (open)
            { U64 d[4];
              for (int c = 0 ; c < 4 ; ++c)
                { const U64 vb = p ? T.off[c][p - 1] + sqField (T.lastCode[p - 1] - 1, c) : st->VB[c];
                  d[c] = T.off[c][t] + sqField (T.firstV[t], c) - vb;
                }
              const U64 startB = p ? T.lastB[p - 1] : st->Bpos, pos = T.firstB[t] - 1;
              if (d[SQ_K] > maxSeq) maxSeq = d[SQ_K];
              if (d[SQ_I] > maxId) maxId = d[SQ_I];
              if (d[SQ_D] > maxDesc) maxDesc = d[SQ_D];
              if (g.fastq && !g.written && d[SQ_K] != d[SQ_Q]) { sqMin64 (&st->errLine, T.firstLine[t] + 1); sqMin64 (&st->errOff, pos); }
              if (!d[SQ_K]) { sqMin64 (&st->stopStart, g.fastq ? startB : startB - 1); sqMin64 (&st->stopEnd, g.fastq ? pos + 1 : pos); }
              if (d[SQ_K] >= SQ_MAXLEN) st->tooLong = 1;
              if (fillMode)                                 /* the bases of earlier windows are the writer's to splice in */
                { const U64 carried = p ? 0 : st->V[SQ_K] - st->VB[SQ_K];
                  fill = (U32) (d[SQ_K] - carried);
                  if (!p) { win->spliceCount = carried; win->spliceTile = t; }
                }
            }
          T.firstFill[t] = fill;
        }
      T.outSum[t] = (U64) T.out[t] + fill;
    }
  __syncthreads ();
  const U64 outBytes = mgGroupScan<MgSum> (T.outSum, T.outOff, nTiles, (U64) 0, lds);
  maxSeq = mgBlockReduce<MG_GROUP_THREADS, MgMax> (maxSeq, lds); maxId = mgBlockReduce<MG_GROUP_THREADS, MgMax> (maxId, lds); maxDesc = mgBlockReduce<MG_GROUP_THREADS, MgMax> (maxDesc, lds);
  if (tid == 0)
    { if (lastTile)
        { const U64 p = lastTile - 1;
          for (int c = 0 ; c < 4 ; ++c) st->VB[c] = T.off[c][p] + sqField (T.lastCode[p] - 1, c);
          st->Bpos = T.lastB[p]; st->bSeen = 1;
        }
      for (int c = 0 ; c < 4 ; ++c) st->V[c] = tot[c];
      if (g.hoco && g.written && !g.fastq) st->lastKept = keptAll;
      if (maxSeq > st->maxSeq) st->maxSeq = maxSeq;
      if (maxId > st->maxId) st->maxId = maxId;
      if (maxDesc > st->maxDesc) st->maxDesc = maxDesc;
      win->outBytes = outBytes;
    }
}

/* ---------------------------------------------------------------------------------------- */
/* host side                                                                                  */

static thread_local U64 gSeqDiag[4];                     /* windows, tiles, records across a window edge, kernel launches */
extern "C" void mgSeqConvertDiag (U64 out4[4]) { memcpy (out4, gSeqDiag, sizeof (gSeqDiag)); }
static thread_local double gSeqMs[8];                    /* (MODGPU_SEED_TIMING=1) the first walk, the second; of both: reading; of the second: device -> page-locked copies, waiting for a block, the writer; the kernels of the first walk, of the second (between events on their stream) */
/* The most output bytes n bytes of text can become (+ 16).  Every byte gives at most one, but: a record start gives the newline that ends the record before it
   and its own marker, while the newline in front of it gave one too if it ended a HEADER line -- a record without a sequence line grows by one byte, and
   there are at most (n + 1) / 2 starts in n bytes; the first byte of a description gives the space as well, where the separator (which gives nothing) may be
   the window before's last byte.  FASTA -> FASTQ: a start gives "\n+\n", the '!' run, "\n@": with s starts at most n - 2 s + 1 bytes are bases, each itself
   and its '!', so 2 n + 2 s + 1 <= 3 n + 2.  FASTQ in: a line gives at most its bytes */
static size_t sqOutCap (size_t n, bool fastqIn, bool fastqOut) { return (fastqIn ? n : fastqOut ? 3 * n : n + n / 2) + 16; }
static size_t sqFill (void *src, unsigned char *dst, size_t cap, U64 off)      /* CpSource::fill, timed */
{ struct timespec t0, t1; clock_gettime (CLOCK_MONOTONIC, &t0);
  const size_t got = CpSource::fill (src, dst, cap, off);
  clock_gettime (CLOCK_MONOTONIC, &t1); gSeqMs[2] += tsMs (t0, t1);
  return got;
}

struct SqPass {                                          /* one walk over the text */
  SqCfg g = { 0, 0, 0, 0 };
  bool write = false, typeError = false;
  int type = 0;
  size_t tilesCap = 0, outCap = 0;
  SqTiles T; SqState *dState = 0; SqWin *dWin = 0; unsigned char *dOut[2] = { 0, 0 };
  TsWriter *wr = 0; MgBgzfSink *bz = 0; hipStream_t copy = 0;      /* the window's output goes to one of the two: as text to the writer thread, or on the device into the BGZF sink */
  U64 pending = SQ_NONE;                                  /* the window whose output is still on the device */
  U32 lastByte = 0; U64 bytes = 0;
  double msCopy = 0, msWait = 0, msKernels = 0;
  hipEvent_t ev[2][2] = { { 0, 0 }, { 0, 0 } }; U64 timed = SQ_NONE;      /* MODGPU_SEED_TIMING=1: events around a window's kernels; the window whose pair is unread */
  void readEvents ()                                       /* (the window loop has waited for that window's kernels) */
  { float ms = 0;
    if (timed != SQ_NONE && hipEventElapsedTime (&ms, ev[timed & 1][0], ev[timed & 1][1]) == hipSuccess) msKernels += ms;
    timed = SQ_NONE;
  }
  /* window k's output to the writer: its kernels are over (the window loop waited for them) */
  int drain (U64 k)
  { SqWin w;
    struct timespec t0, t1, t2;
    if (hipMemcpyAsync (&w, dWin + (k & 1), sizeof (w), hipMemcpyDeviceToHost, copy) != hipSuccess || hipStreamSynchronize (copy) != hipSuccess) return mgHipFail (hipGetLastError (), "mgSeqConvert"), -1;
    if (w.outBytes > outCap || (w.spliceCount && w.spliceAt > w.outBytes))
      { mgSetError ("mgSeqConvert: a window's output of %llu bytes, room for %llu", (unsigned long long) w.outBytes, (unsigned long long) outCap); return -1; }
    if (bz)                                                /* the text stays on the device: the sink deflates it there (mg_bgzfsink.hip) */
      { const U64 at = w.spliceCount ? w.spliceAt : w.outBytes;
        clock_gettime (CLOCK_MONOTONIC, &t0);
        const int rc = mgBgzfSinkAppendDevice (bz, dOut[k & 1], (size_t) at) || (w.spliceCount && mgBgzfSinkAppendRun (bz, '!', w.spliceCount))
                       || mgBgzfSinkAppendDevice (bz, dOut[k & 1] + at, (size_t) (w.outBytes - at));
        clock_gettime (CLOCK_MONOTONIC, &t1); msCopy += tsMs (t0, t1);
        return rc ? -1 : 0;
      }
    clock_gettime (CLOCK_MONOTONIC, &t0);
    TsWriter::Block &b = wr->acquire ();
    clock_gettime (CLOCK_MONOTONIC, &t1);
    if (w.outBytes && (hipMemcpyAsync (b.p, dOut[k & 1], w.outBytes, hipMemcpyDeviceToHost, copy) != hipSuccess || hipStreamSynchronize (copy) != hipSuccess))
      { b.n = 0; b.spliceCount = 0; wr->submit (b); return mgHipFail (hipGetLastError (), "mgSeqConvert"), -1; }
    clock_gettime (CLOCK_MONOTONIC, &t2);
    msWait += tsMs (t0, t1); msCopy += tsMs (t1, t2);
    b.n = (size_t) w.outBytes; b.spliceAt = w.spliceAt; b.spliceCount = w.spliceCount;
    wr->submit (b);
    return 0;
  }
  static int window (void *v, const MgTextWindow *w, void *stream)
  { SqPass *p = (SqPass *) v;
    hipStream_t st = (hipStream_t) stream;
    if (!w->index)
      { p->type = w->first == '>' ? 1 : w->first == '@' ? 2 : 0;
        if (!p->type) { p->typeError = true; return -1; }
        p->g.fastq = p->type == 2;
      }
    const U64 nTiles = (w->n + SQ_TILE - 1) / SQ_TILE;
    if (nTiles > p->tilesCap) { mgSetError ("mgSeqConvert: a window of %llu tiles, room for %llu", (unsigned long long) nTiles, (unsigned long long) p->tilesCap); return -1; }
    const int cur = (int) (w->index & 1);
    const int edge = !w->index ? 0 : (p->g.fastq ? w->prevByte == '\n' : w->first == '>' && w->prevByte == '\n') ? 1 : 2;
    if (p->ev[0][0]) { p->readEvents (); (void) hipEventRecord (p->ev[cur][0], st); }
    hipLaunchKernelGGL (mgSeqFnKernel, dim3 ((unsigned) nTiles), dim3 (SQ_THREADS), 0, st, w->dText, (U64) w->n, w->prevByte, p->g.fastq, p->T.fn, p->T.nl);
    hipLaunchKernelGGL (mgSeqStateScanKernel, dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, p->T, nTiles, p->g.fastq, edge, p->dState);
    hipLaunchKernelGGL (mgSeqTileKernel<0>, dim3 ((unsigned) nTiles), dim3 (SQ_THREADS), 0, st, w->dText, (U64) w->n, w->off, w->prevByte, p->g, p->T, (unsigned char *) 0, (U64) 0, p->dWin + cur, p->dState);
    hipLaunchKernelGGL (mgSeqStitchKernel, dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, p->T, nTiles, p->g, p->dWin + cur, p->dState);
    gSeqDiag[3] += 4;
    if (p->write)
      { if (!p->g.fastq && p->g.outFastq && hipMemsetAsync (p->dOut[cur], '!', p->outCap, st) != hipSuccess) return mgHipFail (hipGetLastError (), "mgSeqConvert"), -1;
        hipLaunchKernelGGL (mgSeqTileKernel<1>, dim3 ((unsigned) nTiles), dim3 (SQ_THREADS), 0, st, w->dText, (U64) w->n, w->off, w->prevByte, p->g, p->T, p->dOut[cur], (U64) p->outCap, p->dWin + cur, p->dState);
        ++gSeqDiag[3];
      }
    if (p->ev[0][0]) { (void) hipEventRecord (p->ev[cur][1], st); p->timed = w->index; }
    if (hipGetLastError () != hipSuccess) return mgFailedWith ("mgSeqConvert: launch failed");
    if (p->write)                                          /* the window before this one leaves while this one is in the kernels */
      { if (p->pending != SQ_NONE && p->drain (p->pending)) return -1;
        p->pending = w->index;
      }
    p->lastByte = w->last; p->bytes = w->off + w->n;
    gSeqDiag[1] += nTiles;
    return 0;
  }
};

/* the text of `src` below src.limit through the kernels; the second walk writes to `out`, or appends to `bz`.  0 / -1 */
static int sqWalk (CpSource &src, const SqCfg &g, FILE *out, MgBgzfSink *bz, SqState *S, int *type, U32 *lastByte, U64 *bytes)
{
  MgDevScratch scratch ("mgSeqConvert");
  SqPass p; p.g = g; p.write = out != 0 || bz != 0; p.bz = bz;
  const size_t hint = (size_t) src.size < TS_WINDOW_HINT ? (size_t) src.size : TS_WINDOW_HINT, window = mgTextWindowBytes (hint);
  p.tilesCap = window / SQ_TILE + 2;
  U64 *block = 0;
  if (scratch.get (&p.dState, 1) || scratch.get (&p.dWin, 2) || scratch.get (&block, (size_t) SQ_TILE_ARRAYS * p.tilesCap)) return -1;
  { U64 *q = block; size_t k = 0;
    auto next = [&] () { U64 *r = q + k * p.tilesCap; ++k; return r; };
    SqTiles &T = p.T;
    T.fn = (U32 *) next (); T.nl = (U32 *) next (); T.state = (U32 *) next (); T.line = next ();
    for (int c = 0 ; c < 4 ; ++c) { T.cnt[c] = (U32 *) next (); T.off[c] = next (); }
    T.lastCode = next (); T.firstV = next (); T.lastB = next (); T.firstB = next (); T.firstLine = next ();
    T.out = (U32 *) next (); T.firstFill = (U32 *) next (); T.outSum = next (); T.outOff = next ();
    T.lastKept = next (); T.keptIn = next (); T.firstKept = (U32 *) next (); T.prevTile = next ();
    if (k != SQ_TILE_ARRAYS) { mgSetError ("mgSeqConvert: %d tile arrays, %d named", SQ_TILE_ARRAYS, (int) k); return -1; }
  }
  memset (S, 0, sizeof (*S));
  S->errLine = S->errOff = S->badOff = S->nulOff = S->badLine = S->stopStart = S->stopEnd = SQ_NONE;
  if (hipMemcpy (p.dState, S, sizeof (*S), hipMemcpyHostToDevice) != hipSuccess) { scratch.fail (); return -1; }
  TsWriter wr;
  if (p.write)
    { p.outCap = sqOutCap (window, g.fastq != 0, g.outFastq != 0);
      if (scratch.get (&p.dOut[0], p.outCap) || scratch.get (&p.dOut[1], p.outCap)) return -1;
      if (hipStreamCreateWithFlags (&p.copy, hipStreamNonBlocking) != hipSuccess) { scratch.fail (); return -1; }
      if (!bz && wr.open (out, p.outCap)) { wr.close (); (void) hipStreamDestroy (p.copy); return -1; }
      p.wr = &wr;
    }
  U64 nWindows = 0;
  struct timespec t0, t1; clock_gettime (CLOCK_MONOTONIC, &t0);
  if (mgKnobs ()->seedTiming == 1)
    for (int i = 0 ; i < 4 ; ++i) if (hipEventCreate (&p.ev[i >> 1][i & 1]) != hipSuccess) { (void) hipGetLastError (); p.ev[0][0] = 0; break; }
  int rc = src.walk (hint, sqFill, SqPass::window, &p, &nWindows);
  if (p.ev[0][0]) { if (!rc) p.readEvents (); gSeqMs[p.write ? 7 : 6] += p.msKernels; }
  for (int i = 0 ; i < 4 ; ++i) if (p.ev[i >> 1][i & 1]) (void) hipEventDestroy (p.ev[i >> 1][i & 1]);
  gSeqDiag[0] += nWindows;
  if (p.write)
    { if (!rc && p.pending != SQ_NONE && p.drain (p.pending)) rc = -1;
      if (!bz && wr.close () && !rc) { mgSetError ("mgSeqConvert: write failed"); rc = -1; }
      (void) hipStreamDestroy (p.copy);
      gSeqMs[3] += p.msCopy; gSeqMs[4] += p.msWait; gSeqMs[5] += wr.msWrite;
    }
  clock_gettime (CLOCK_MONOTONIC, &t1); gSeqMs[p.write ? 1 : 0] += tsMs (t0, t1);
  if (p.typeError) { mgSetError ("sequence file %s is neither FASTA nor FASTQ text", src.name ? src.name : "(text)"); return -1; }
  if (rc) return -1;
  if (!nWindows) { mgSetError ("sequence file %s unreadable or empty", src.name ? src.name : "(text)"); return -1; }
  if (hipMemcpy (S, p.dState, sizeof (*S), hipMemcpyDeviceToHost) != hipSuccess) { scratch.fail (); return -1; }
  gSeqDiag[2] += S->crossed;
  *type = p.type; *lastByte = p.lastByte; *bytes = p.bytes;
  return 0;
}

static int sqConvert (CpSource &src, int flags, TsSink &sink, FILE *err, MgSeqConvert *res)
{
  typedef unsigned long long ull;
  memset (gSeqDiag, 0, sizeof (gSeqDiag)); memset (gSeqMs, 0, sizeof (gSeqMs)); mgInflateDiagReset (); mgGunzipDiagReset ();
  if (mgEnsureDevice ()) return -1;
  SqCfg g = { 0, (flags & MG_SEQ_FASTQ) != 0, (flags & MG_SEQ_HOCO) != 0, 0 };
  SqState S; int type = 0; U32 lastByte = 0; U64 textEnd = 0;
  /* the first walk: is the text acceptable, and where does what is written end */
  if (sqWalk (src, g, 0, 0, &S, &type, &lastByte, &textEnd)) return -1;
  const bool fastq = type == 2;
  const bool complete = fastq ? lastByte == '\n' && !(S.line & 3) : lastByte == '\n' && S.hdrEnd != textEnd;
  const U64 cut = fastq ? S.Bpos : S.Bpos - 1;            /* the byte after the last complete record (FASTQ) / where the text's last record starts (FASTA: its first byte is a start) */
  if (!fastq && complete && S.bSeen)                        /* the FASTA record that the text's end ends */
    { const U64 len = S.V[SQ_K] - S.VB[SQ_K];
      if (len >= SQ_MAXLEN) S.tooLong = 1;
      if (!len && S.stopStart == SQ_NONE) { S.stopStart = S.Bpos - 1; S.stopEnd = textEnd; }
    }
  const bool stop = g.hoco && S.stopStart != SQ_NONE;      /* seqhoco.c:26: neither that record nor any after it is read */
  const U64 endRead = stop ? S.stopEnd : complete ? textEnd : cut, endRule = stop ? S.stopEnd : textEnd;
  const U64 firstBad = S.badOff < S.nulOff ? S.badOff : S.nulOff;
  const bool rule = S.errOff != SQ_NONE && S.errOff < endRule, bad = firstBad != SQ_NONE && firstBad < endRead;
  if (rule && (!bad || !fastq || (S.errLine - 1) / 4 <= (S.badLine - 1) / 4))
    { const char *what = (S.errLine & 3) == 1 ? "no initial @ for FASTQ record line" : (S.errLine & 3) == 3 ? "missing + FASTQ line" : "qual not same length as seq line";
      mgSetError ("%s %llu", what, (ull) S.errLine);
      return -1;
    }
  if (bad)
    { if (S.nulOff < S.badOff) mgSetError ("NUL byte at offset %llu of a header line (the reference's strlen would cut the name there)", (ull) S.nulOff);
      else mgSetError ("byte at offset %llu of the %s is outside the reference's tables (%s would index them out of bounds)", (ull) S.badOff,
                       fastq ? "FASTQ sequence lines" : "FASTA sequence lines", g.hoco ? "seqhoco" : "seqconvert");
      return -1;
    }
  if (S.tooLong) { mgSetError ("a record of 2^31 bases or more: the reference's lengths are int"); return -1; }
  char errText[96] = "";
  if (!complete && !stop) snprintf (errText, sizeof (errText), "incomplete sequence record line %llu\n", (ull) (S.line + 1));      /* seqio.c:215-219: the record is dropped */
  const U64 limit = stop ? S.stopStart : complete ? textEnd : cut;
  MgSeqConvert r; memset (&r, 0, sizeof (r));
  r.inType = type; r.outType = g.outFastq ? 2 : 1;
  /* the second walk: the records that are written */
  sink.textHint = limit;                                   /* (a short text gets a short row in the BGZF sink) */
  FILE *out = sink.get ();
  if (!out) return -1;
  if (limit)
    { src.limit = limit;
      g.written = 1; g.fastq = fastq;                      /* (the output buffers are sized by it) */
      if (src.reopen () || sqWalk (src, g, sink.device () ? 0 : out, sink.device (), &S, &type, &lastByte, &textEnd)) return -1;
      U64 maxSeq = S.maxSeq, maxId = S.maxId, maxDesc = S.maxDesc;
      if (!fastq)                                           /* the record that the text's end ends: its two newlines, and its '!' */
        { const U64 len = S.V[SQ_K] - S.VB[SQ_K], id = S.V[SQ_I] - S.VB[SQ_I], desc = S.V[SQ_D] - S.VB[SQ_D];
          if (len > maxSeq) maxSeq = len;
          if (id > maxId) maxId = id;
          if (desc > maxDesc) maxDesc = desc;
          if (MgBgzfSink *bz = sink.device ())
            { if (mgBgzfSinkAppendHost (bz, "\n", 1) || (g.outFastq && (mgBgzfSinkAppendHost (bz, "+\n", 2) || mgBgzfSinkAppendRun (bz, '!', len) || mgBgzfSinkAppendHost (bz, "\n", 1)))) return -1; }
          else
            { bool ok = fputc ('\n', out) != EOF;
              if (ok && g.outFastq) ok = fputs ("+\n", out) != EOF && TsWriter::bangs (out, len) && fputc ('\n', out) != EOF;
              if (!ok) { mgSetError ("mgSeqConvert: write failed"); return -1; }
            }
        }
      r.nSeq = r.nSeqIn = S.nRec; r.totSeqLen = S.V[SQ_K]; r.maxSeqLen = maxSeq; r.totIdLen = S.V[SQ_I]; r.totDescLen = S.V[SQ_D]; r.maxIdLen = maxId; r.maxDescLen = maxDesc;
      r.totSeqLenIn = S.totFilt;
    }
  if (mgKnobs ()->seedTiming == 1)
    fprintf (stderr, "mgSeqConvert: first walk %.1f ms, second walk %.1f ms; reading %.1f ms, device -> page-locked copies %.1f ms, waiting for a block %.1f ms, writer %.1f ms, kernels %.1f ms + %.1f ms\n",
             gSeqMs[0], gSeqMs[1], gSeqMs[2], gSeqMs[3], gSeqMs[4], gSeqMs[5], gSeqMs[6], gSeqMs[7]);
  if (err && errText[0]) fputs (errText, err);
  if (res) *res = r;
  return 0;
}

static int sqFlags (int flags, const char *what)
{
  if (flags & ~(MG_SEQ_FASTA | MG_SEQ_FASTQ | MG_SEQ_HOCO)) { mgSetError ("%s: unknown flags %d", what, flags); return -1; }
  if ((flags & MG_SEQ_FASTA) && (flags & MG_SEQ_FASTQ)) { mgSetError ("%s: MG_SEQ_FASTA and MG_SEQ_FASTQ at once", what); return -1; }
  if ((flags & MG_SEQ_HOCO) && (flags & MG_SEQ_FASTQ)) { mgSetError ("%s: MG_SEQ_HOCO writes FASTA (seqhoco.c:24), MG_SEQ_FASTQ with it is refused", what); return -1; }
  return 0;
}

extern "C" int mgSeqConvertText (const char *text, U64 n, int flags, FILE *out, FILE *err, MgSeqConvert *res)
{
  if (res) memset (res, 0, sizeof (*res));
  if (sqFlags (flags, "mgSeqConvertText")) return -1;
  if (!flags) { mgSetError ("mgSeqConvertText: no output type: MG_SEQ_FASTA, MG_SEQ_FASTQ or MG_SEQ_HOCO (the program would write its binary format)"); return -1; }
  if (!out) { mgSetError ("mgSeqConvertText: no output"); return -1; }
  if (!text || !n) { mgSetError ("sequence text unreadable or empty"); return -1; }
  CpSource src; src.mem = (const unsigned char *) text; src.size = n;
  TsSink sink; sink.f = out;
  const int rc = sqConvert (src, flags, sink, err, res);
  if (!rc && fflush (out)) { mgSetError ("mgSeqConvertText: write failed"); return -1; }
  return rc;
}

/* mgSeqConvertFile and mgSeqConvertFileBgzf: they differ in where the second walk's output goes, and in that the latter's type suffix may stand before .bgz too */
static int sqConvertFile (const char *inName, const char *outName, int flags, FILE *err, MgSeqConvert *res, bool bgzf)
{
  if (res) memset (res, 0, sizeof (*res));
  if (sqFlags (flags, "mgSeqConvertFile")) return -1;
  if (!inName || !outName) { mgSetError ("mgSeqConvertFile: no file name"); return -1; }
  TsSink sink; sink.name = outName; sink.bgzf = bgzf;
  sink.toStdout = !strcmp (outName, "-") || (!bgzf && !strcmp (outName, "-z"));
  size_t len = strlen (outName);
  const bool gzName = !sink.toStdout && len > 3 && !strcmp (outName + len - 3, ".gz"), bgzName = bgzf && !sink.toStdout && len > 4 && !strcmp (outName + len - 4, ".bgz");
  sink.gz = !bgzf && (!strcmp (outName, "-z") || gzName);
  if (!(flags & (MG_SEQ_FASTA | MG_SEQ_FASTQ | MG_SEQ_HOCO)))      /* seqio.c:426-428 */
    { if (gzName) len -= 3; else if (bgzName) len -= 4;
      if (!sink.toStdout && len > 3 && !strncmp (outName + len - 3, ".fa", 3)) flags |= MG_SEQ_FASTA;
      else if (!sink.toStdout && len > 3 && !strncmp (outName + len - 3, ".fq", 3)) flags |= MG_SEQ_FASTQ;
      else
        { mgSetError ("mgSeqConvertFile: no output type from the flags or from a .fa / .fq%s suffix of %s (the program would write its binary format)", sink.gz || gzName ? " before .gz" : bgzName ? " before .bgz" : "", outName);
          return -1;
        }
    }
  CpSource src;
  if (src.open (inName)) { src.close (); return -1; }
  mgDeflateDiagReset ();
  int rc = sqConvert (src, flags, sink, err, res);
  src.close ();
  return sink.close (rc);
}
extern "C" int mgSeqConvertFile (const char *inName, const char *outName, int flags, FILE *err, MgSeqConvert *res) { return sqConvertFile (inName, outName, flags, err, res, false); }
extern "C" int mgSeqConvertFileBgzf (const char *inName, const char *outName, int flags, FILE *err, MgSeqConvert *res) { return sqConvertFile (inName, outName, flags, err, res, true); }
