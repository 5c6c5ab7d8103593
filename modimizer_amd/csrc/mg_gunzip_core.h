/* mg_gunzip_core.h — ordinary gzip (RFC 1952: one deflate stream a member, no block table) inflated in parallel, written once for host and device.
 *
 * It sits beside mg_inflate_core.h and uses its bit reader, mgiBuild, mgiDecode, mgiBlockCodes, mgiStoredHeader, mgiLength, mgiDistance and the CRC slice and combine arithmetic.  No zlib, no
 * allocation, plain C that is also C++ / HIP: mg_gunzip.hip compiles the stages for gfx950 and the whole of it for the host (mgGunzipHost);
 * tools/gunzip_host_check.c includes nothing else.
 *
 * The method is the one pugz and rapidgzip use on CPUs.  The compressed bytes from a known block start on are cut into CHUNKS of equal size, a BATCH of
 * them at a time:
 *   find     the first bit offset inside a chunk at which a non-final dynamic block can start (mgzCheap on the header's bits, then mgzVerify on the
 *            code tables): the chunk's CANDIDATE.  Chunk 0 starts at the known position and is not searched.  A chunk without a candidate is FOLDED
 *            into its predecessor, whose decoder simply runs through it;
 *   decode   every chunk from its candidate to the first block boundary at or past the next candidate, into 16-bit SYMBOLS: a literal is 0 .. 255, a
 *            reference that reaches before the chunk's own output is 0x8000 | k, k the place in the 32 KiB window before the chunk (mgzChunkDecode);
 *   chain    chunk i + 1 is CONFIRMED if and only if chunk i is confirmed and ended exactly on chunk i + 1's candidate; chunk 0 is confirmed by
 *            definition.  By induction every confirmed start is a true block start, and the symbols of a confirmed chunk are what a serial decoder
 *            produces there.  The first chunk that breaks the chain ends the batch, the chunks behind it are DISCARDED, and the next batch starts at
 *            the end position of the last confirmed chunk, which is a true block start again: every batch confirms at least its first chunk, so the
 *            stream always moves on (mgzChainStep);
 *   windows  the window after chunk i is the window before it and the last 32 768 symbols of its output (mgzWindowSym), carried in chunk order;
 *   resolve  symbols and the window before the chunk become bytes, and the chunk's CRC-32 is folded with x^(8 * bytes after) (mgzResolveSlice).
 * Members (mgzNext): the gzip header is parsed, after a final block the trailer is checked (CRC-32, ISIZE mod 2^32) and the next header follows, with an
 * empty window.  The symbols a chunk may write are a guess: a chunk that overflows ends its batch's chain and starts the next batch with twice the room.
 *
 * BOUNDS.  Every read of the compressed bytes is clamped below their end (mgzLoad64, the bit reader of mg_inflate_core.h); a chunk writes symbols
 * [0, cap) of its own stretch and nothing else (MGZ_CAPACITY otherwise); a marker indexes the 32 KiB window, which is always that long.
 */
#ifndef MG_GUNZIP_CORE_H
#define MG_GUNZIP_CORE_H
#include "mg_inflate_core.h"

enum { MGZ_CAPACITY = 9,     /* a chunk's symbols exceed the room it was given (not MGI_OUTPUT: the stream may be fine) */
       MGZ_HEADER = 10 };    /* not a gzip header where one must be */

#define MGZ_WINDOW 32768u
#define MGZ_NONE (~(uint64_t) 0)
#define MGZ_SYM_MAX ((uint32_t) 1 << 28)      /* the most symbols a single chunk is ever given */
#define MGZ_MIN_CHUNK 4096u

/* one chunk of a batch */
typedef struct {
  uint64_t cand;             /* bit position of its candidate in the compressed bytes; MGZ_NONE: folded */
  uint64_t end;              /* where its decode ended */
  uint64_t off;              /* its text's place in the batch's output (set by the chain) */
  uint32_t nSym, status, final, ok;      /* ok: confirmed and decoded, so resolved */
  uint32_t wlen, pad;        /* bytes of the window before it that belong to the member */
} MgzChunk;

/* why a batch's chain ended */
enum { MGZ_END = 0,          /* the batch's chunks are all confirmed */
       MGZ_FINAL = 1,        /* a final block: the member's trailer follows at `next` */
       MGZ_BROKE = 2,        /* a chunk did not end on its successor's candidate */
       MGZ_RETRY = 3,        /* a confirmed chunk overflowed: it starts the next batch */
       MGZ_ERROR = 4 };      /* a confirmed chunk does not decode, or the output is full: the stream is wrong at errBit */

/* what a batch reports (all 64-bit: one copy from the device) */
typedef struct {
  uint64_t confirmed, discarded, folded;      /* chunks, as mgGunzipDiag counts them */
  uint64_t outBytes;         /* text of the confirmed chunks */
  uint64_t next;             /* bit position the stream continues at */
  uint64_t reason, status, errBit;
  uint64_t crc;              /* of the batch's text (resolve) */
  uint64_t badMarker;        /* resolve: the lowest candidate of a chunk with a marker below the member's start; MGZ_NONE: none */
  uint64_t wlenAfter, carrySlot;      /* the window the stream continues with: its valid bytes and which of the batch's windows it is */
} MgzSummary;

/* ---------------------------------------------------------------------------------------------------------------- loads and seeks */
/* the 8 bytes at `byte`, those past the end read as 0 */
MGI_HD uint64_t mgzLoad64 (const uint8_t *comp, uint64_t n, uint64_t byte)
{
  uint64_t v = 0;
  if (byte + 8 <= n) { __builtin_memcpy (&v, comp + byte, 8); return v; }
  { uint32_t i; for (i = 0 ; i < 8 && byte + i < n ; ++i) v |= (uint64_t) comp[byte + i] << (8 * i); }
  return v;
}
/* the reader at bit position `bit` of comp[0 .. n) (bit <= 8 n) */
MGI_HD void mgzSeek (MgInfBits *b, const uint8_t *comp, uint64_t n, uint64_t bit)
{
  const uint64_t byte = bit >> 3, left = n - byte;
  uint32_t v;
  b->in = comp + byte; b->n = left > 0xfffffff0u ? 0xfffffff0u : (uint32_t) left;
  b->pos = 0; b->cnt = 0; b->buf = 0; b->ahead = 0;
  mgiPrime (b);
  if (bit & 7) (void) mgiBits (b, (uint32_t) (bit & 7), &v);
}
MGI_HD uint64_t mgzTell (const MgInfBits *b, const uint8_t *comp) { return ((uint64_t) (b->in - comp) + b->pos) * 8 - b->cnt; }

/* ---------------------------------------------------------------------------------------------------------------- the candidate test */
/* the cheap part, in registers.  lo: the 64 bits from the offset on, hi: the 64 behind them.  BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, and the
   HCLEN + 4 lengths of the code-length code make a complete code: the sum of 2^(7 - l) over the l > 0 is 128 */
MGI_HD int mgzCheap (uint64_t lo, uint64_t hi)
{
  uint32_t ncode, i, sum = 0;
  if ((lo & 7) != 4) return 0;
  if (((lo >> 3) & 31) > 29 || ((lo >> 8) & 31) > 29) return 0;
  ncode = (uint32_t) ((lo >> 13) & 15) + 4;
  for (i = 0 ; i < ncode ; ++i)
    { const uint32_t o = 17 + 3 * i;
      const uint32_t l = (uint32_t) (o < 62 ? lo >> o : o >= 64 ? hi >> (o - 64) : (lo >> o) | (hi << (64 - o))) & 7;
      if (l) sum += 128u >> l;
    }
  return sum == 128;
}
/* the bits at offset `bit` for mgzCheap, from two loads */
MGI_HD int mgzCheapAt (const uint8_t *comp, uint64_t n, uint64_t bit)
{
  const uint64_t w0 = mgzLoad64 (comp, n, bit >> 3), w1 = mgzLoad64 (comp, n, (bit >> 3) + 8);
  const uint32_t s = (uint32_t) (bit & 7);
  const uint64_t lo = s ? (w0 >> s) | (w1 << (64 - s)) : w0, hi = w1 >> s;
  return mgzCheap (lo, hi);
}
/* the full part, on the team's tables: the lengths read, a complete literal/length code with an end-of-block code, a distance code that is complete or has
   at most one code (stricter than what a decoder accepts: zlib's encoder writes nothing else) */
MGI_HD int mgzVerify (const uint8_t *comp, uint64_t n, uint64_t bit, MgInfTables *T)
{
  MgInfBits b;
  uint32_t v, len, codes = 0;
  int left = 1;
  mgzSeek (&b, comp, n, bit);
  if (!mgiBits (&b, 3, &v) || v != 4) return 0;
  if (mgiBlockCodes (&b, 2, T, 0)) return 0;
  for (len = 1 ; len < 16 ; ++len) { left <<= 1; left -= (int) T->lcount[len]; }
  if (left) return 0;
  left = 1;
  for (len = 1 ; len < 16 ; ++len) { left <<= 1; left -= (int) T->dcount[len]; codes += T->dcount[len]; }
  return !left || codes <= 1;
}
/* the first candidate in bits [lo, hi), one offset after the other (the host's finder; the kernel tests 64 at a time and verifies in the same order) */
MGI_HD uint64_t mgzFindSerial (const uint8_t *comp, uint64_t n, uint64_t lo, uint64_t hi, MgInfTables *T)
{
  uint64_t p;
  for (p = lo ; p < hi ; ++p) if (mgzCheapAt (comp, n, p) && mgzVerify (comp, n, p, T)) return p;
  return MGZ_NONE;
}
/* the bits chunk c of a batch that starts at `start` is searched in: [*lo, *hi), clipped to the compressed bytes */
MGI_HD void mgzChunkRange (uint64_t start, uint32_t chunkBytes, uint32_t c, uint64_t n, uint64_t *lo, uint64_t *hi)
{
  const uint64_t base = start >> 3;
  *lo = (base + (uint64_t) c * chunkBytes) * 8; *hi = *lo + (uint64_t) chunkBytes * 8;
  if (*lo > n * 8) *lo = n * 8;
  if (*hi > n * 8) *hi = n * 8;
}
/* where chunk c's decode may stop: the candidate of the next chunk that has one, else the batch's end */
MGI_HD uint64_t mgzStopOf (const MgzChunk *ch, uint32_t nChunks, uint32_t c, uint64_t batchEnd)
{
  uint32_t k;
  for (k = c + 1 ; k < nChunks ; ++k) if (ch[k].cand != MGZ_NONE) return ch[k].cand;
  return batchEnd;
}

/* ---------------------------------------------------------------------------------------------------------------- a chunk's decode */
/* Blocks from bit position `start` up to the first block boundary at or past `stop` (or a final block) into out[0 .. cap).  known: the bytes of the window
   before this chunk that belong to the member, if that is known (chunk 0 of a batch) -- a reference below them is MGI_DISTANCE -- or ~0.  Returns a status;
   *end, *nSym and *final are set on every return (the position and the symbols reached). */
MGI_HD uint32_t mgzChunkDecode (const uint8_t *comp, uint64_t n, uint64_t start, uint64_t stop, uint32_t known, uint16_t *out, uint32_t cap, MgInfTables *T,
                                uint64_t *end, uint32_t *nSym, uint32_t *final)
{
  MgInfBits bits, *b = &bits;
  uint32_t o = 0, last = 0, type = 0, st = MGI_OK;
  uint64_t *stats = 0;
  mgzSeek (b, comp, n, start);
  do
    { if (!mgiBits (b, 1, &last) || !mgiBits (b, 2, &type)) { st = MGI_INPUT; break; }
      if (type == 3) { st = MGI_BLOCKTYPE; break; }
      if (type == 0)
        { uint32_t len, i;
          { const int h = mgiStoredHeader (b); if (h < 0) { st = (uint32_t) -h; break; } len = (uint32_t) h; }
          if (len > cap - o) { st = MGZ_CAPACITY; break; }
          for (i = 0 ; i < len ; ++i) out[o + i] = b->in[b->pos + i];
          o += len; b->pos += len;
          mgiPrime (b);
          continue;
        }
      st = mgiBlockCodes (b, type, T, stats);
      if (st) break;
      for (;;)
        { int s = mgiDecode (b, T->lfast, MGI_LBITS, T->lcount, T->lsym);
          uint32_t len, dist, i;
          if (s < 0) { st = s == -2 ? MGI_INPUT : MGI_SYMBOL; break; }
          if (s < 256) { if (o >= cap) { st = MGZ_CAPACITY; break; } out[o++] = (uint16_t) s; continue; }
          if (s == 256) break;
          st = mgiLength (b, s, &len);
          if (!st) st = mgiDistance (b, T, &dist);
          if (st) break;
          if (dist > o && known != ~(uint32_t) 0 && dist - o > known) { st = MGI_DISTANCE; break; }
          if (len > cap - o) { st = MGZ_CAPACITY; break; }
          /* the copy, by the thread that wrote what it reads.  A place before the chunk's output is a marker: window place 32768 - (dist - o) + i; a
             marker that is copied stays a marker, also where dist < len repeats what this copy wrote */
          if (dist <= o && dist >= 4)
            { uint64_t w;
              for (i = 0 ; i + 4 <= len ; i += 4) { __builtin_memcpy (&w, out + o + i - dist, 8); __builtin_memcpy (out + o + i, &w, 8); }
              for ( ; i < len ; ++i) out[o + i] = out[o + i - dist];
            }
          else if (dist <= o)                            /* a run of period 1 .. 3: the period is read once, nothing written is read back */
            { uint16_t per[3];
              uint32_t k = 0;
              for (i = 0 ; i < dist ; ++i) per[i] = out[o - dist + i];
              for (i = 0 ; i < len ; ++i) { out[o + i] = per[k]; if (++k == dist) k = 0; }
            }
          else
            for (i = 0 ; i < len ; ++i)
              out[o + i] = o + i >= dist ? out[o + i - dist] : (uint16_t) (0x8000u | (MGZ_WINDOW - (dist - (o + i))));
          o += len;
        }
      if (st) break;
    }
  while (!last && mgzTell (b, comp) < stop);
  *end = mgzTell (b, comp); *nSym = o; *final = st ? 0 : last;
  return st;
}

/* ---------------------------------------------------------------------------------------------------------------- chain, windows, resolve */
/* One step of the chain walk, by one thread: chunk c is confirmed.  It is accounted for in S, and the return is the chunk the walk goes on with, or
   nChunks if the chain ends here (S->reason says why).  outCap: the room the batch's text has.  Before the first step: mgzChainBegin. */
MGI_HD void mgzChainBegin (MgzSummary *S, uint64_t start, uint32_t wlen)
{
  S->confirmed = S->discarded = S->folded = S->outBytes = 0;
  S->next = start; S->reason = MGZ_END; S->status = MGI_OK; S->errBit = 0; S->crc = 0; S->badMarker = MGZ_NONE;
  S->wlenAfter = wlen; S->carrySlot = 0;
}
MGI_HD uint32_t mgzChainStep (MgzChunk *ch, uint32_t nChunks, uint32_t c, uint64_t outCap, MgzSummary *S)
{
  MgzChunk *k = ch + c;
  uint32_t nx, j;
  k->ok = 0; k->off = S->outBytes; k->wlen = (uint32_t) S->wlenAfter;
  S->carrySlot = c;
  if (k->status == MGZ_CAPACITY) { S->reason = MGZ_RETRY; S->next = k->cand; return nChunks; }
  if (k->status == MGI_OK && k->nSym > outCap - S->outBytes) k->status = MGI_OUTPUT;
  if (k->status) { S->reason = MGZ_ERROR; S->status = k->status; S->errBit = k->end; S->next = k->cand; return nChunks; }
  k->ok = 1; ++S->confirmed;
  S->outBytes += k->nSym; S->next = k->end;
  S->wlenAfter = S->wlenAfter + k->nSym > MGZ_WINDOW ? MGZ_WINDOW : S->wlenAfter + k->nSym;
  for (nx = c + 1 ; nx < nChunks && ch[nx].cand == MGZ_NONE ; ++nx) ;
  S->carrySlot = nx;                                     /* the window after chunk c: that of the next chunk with a candidate, or slot nChunks */
  if (k->final) { S->reason = MGZ_FINAL; S->carrySlot = nChunks; return nChunks; }
  S->folded += nx - (c + 1);
  if (nx == nChunks) { S->reason = MGZ_END; return nChunks; }
  if (ch[nx].cand == k->end) return nx;
  S->reason = MGZ_BROKE; S->carrySlot = nChunks;
  for (j = nx ; j < nChunks ; ++j) if (ch[j].cand == MGZ_NONE) ++S->folded; else ++S->discarded;
  return nChunks;
}
/* byte j of the window after a chunk of nSym symbols, from the window before it (valid in its last wlen bytes; the rest reads as it is) */
MGI_HD uint8_t mgzWindowSym (const uint8_t *before, const uint16_t *sym, uint32_t nSym, uint32_t j)
{
  if (nSym >= MGZ_WINDOW || j >= MGZ_WINDOW - nSym)
    { const uint16_t s = sym[nSym - (MGZ_WINDOW - j)];
      return s & 0x8000u ? before[s & 0x7fffu] : (uint8_t) s;
    }
  return before[j + nSym];
}
/* symbols [a, e) of a chunk into bytes out[a .. e); returns their CRC-32 (finished, as crc32 () gives it); *bad is set if a marker lies below the member's
   start (the window before the chunk has wlen valid bytes) */
MGI_HD uint32_t mgzResolveSlice (const uint32_t *tab, const uint16_t *sym, const uint8_t *win, uint32_t wlen, uint32_t a, uint32_t e, uint8_t *out, uint32_t *bad)
{
  uint32_t c = 0xffffffffu, i;
  for (i = a ; i < e ; ++i)
    { const uint16_t s = sym[i];
      uint8_t v = (uint8_t) s;
      if (s & 0x8000u) { const uint32_t k = s & 0x7fffu; if (k < MGZ_WINDOW - wlen) *bad = 1; v = win[k]; }
      out[i] = v;
      c = tab[(c ^ v) & 0xff] ^ (c >> 8);
    }
  return c ^ 0xffffffffu;
}
/* crc (A B) from crc (A), crc (B) and |B| < 2^32 */
MGI_HD uint32_t mgzCrcAppend (uint32_t crcA, uint32_t crcB, uint32_t lenB) { return mgiMulModP (mgiXPow8 (lenB), crcA) ^ crcB; }

/* ---------------------------------------------------------------------------------------------------------------- a gzip header */
/* the length of the member header at p[0 .. n) into *len: 0; 1 = it does not end within n bytes; 2 = not a gzip header.  *bc: it carries a 'BC' subfield */
MGI_HD int mgzHeader (const uint8_t *p, uint64_t n, uint64_t *len, int *bc)
{
  uint64_t at = 10;
  uint32_t flg;
  *bc = 0;
  if (n >= 1 && p[0] != 0x1f) return 2;
  if (n >= 2 && p[1] != 0x8b) return 2;
  if (n >= 3 && p[2] != 8) return 2;
  if (n >= 4 && (p[3] & 0xe0)) return 2;
  if (n < 10) return 1;
  flg = p[3];
  if (flg & 4)
    { uint64_t xlen, q;
      if (n < at + 2) return 1;
      xlen = (uint64_t) p[at] | ((uint64_t) p[at + 1] << 8); at += 2;
      if (n < at + xlen) return 1;
      for (q = at ; q + 4 <= at + xlen ; q += 4 + ((uint64_t) p[q + 2] | ((uint64_t) p[q + 3] << 8))) if (p[q] == 'B' && p[q + 1] == 'C') *bc = 1;
      at += xlen;
    }
  if (flg & 8) { while (at < n && p[at]) ++at; if (at >= n) return 1; ++at; }
  if (flg & 16) { while (at < n && p[at]) ++at; if (at >= n) return 1; ++at; }
  if (flg & 2)                                            /* FHCRC: the low half of the CRC-32 of the header before it, as zlib checks it */
    { uint32_t c = 0xffffffffu, k;
      uint64_t i;
      if (n < at + 2) return 1;
      for (i = 0 ; i < at ; ++i) { c ^= p[i]; for (k = 0 ; k < 8 ; ++k) c = (c & 1) ? (c >> 1) ^ MGI_POLY : c >> 1; }
      if (((c ^ 0xffffffffu) & 0xffffu) != ((uint32_t) p[at] | ((uint32_t) p[at + 1] << 8))) return 2;
      at += 2;
    }
  *len = at;
  return 0;
}

/* ---------------------------------------------------------------------------------------------------------------- the stream (host side of both compiles) */
/* what one batch is asked to do */
typedef struct { uint64_t start; uint32_t wlen, nChunks, chunkBytes, cap, first; uint64_t outCap; } MgzPlan;      /* first: the batch begins a member */

/* diag: chunks speculated, confirmed, discarded after a chain break, folded (no candidate), batches, members, capacity retries, kernel launches */
enum { MGZ_D_SPEC = 0, MGZ_D_CONF = 1, MGZ_D_DISC = 2, MGZ_D_FOLD = 3, MGZ_D_BATCH = 4, MGZ_D_MEMBER = 5, MGZ_D_RETRY = 6, MGZ_D_LAUNCH = 7 };
#define MGZ_LAUNCHES 4       /* a batch: find, decode, chain, resolve */

typedef struct {
  uint64_t n;                /* compressed bytes */
  uint32_t chunkBytes, batchChunks, baseCap, cap;
  uint64_t pos;              /* bit position: the next batch's start inside a member, the next header's first bit between members */
  int inMember, done;
  uint32_t wlen, crc;
  uint64_t memberBytes, produced, outCap;
  uint32_t status; uint64_t errOff;      /* on failure: the status and the compressed byte it was met at */
  uint64_t diag[8];
} MgzStream;

/* peek: up to n bytes of the compressed file at `off` into buf, returns how many.  batch: runs plan P (find, decode, chain, windows, resolve), appends the
   text to wherever the caller keeps it and fills S; non-zero if it could not run */
typedef uint32_t (*MgzPeekFn) (void *ctx, uint64_t off, uint8_t *buf, uint32_t n);
typedef int (*MgzBatchFn) (void *ctx, const MgzPlan *P, MgzSummary *S);

static inline void mgzStreamInit (MgzStream *s, uint64_t n, uint32_t chunkBytes, uint32_t batchChunks, uint32_t symbolsPerChunk, uint64_t outCap)
{
  uint32_t i;
  s->n = n;
  s->chunkBytes = chunkBytes < MGZ_MIN_CHUNK ? MGZ_MIN_CHUNK : chunkBytes;
  s->batchChunks = batchChunks ? batchChunks : 1;
  s->baseCap = symbolsPerChunk ? symbolsPerChunk : 1;
  if (s->baseCap > MGZ_SYM_MAX) s->baseCap = MGZ_SYM_MAX;
  while ((uint64_t) s->batchChunks * s->baseCap > 0xf0000000u) s->batchChunks = (s->batchChunks + 1) / 2;      /* a batch's text stays below 2^32 bytes */
  s->cap = s->baseCap;
  s->pos = 0; s->inMember = 0; s->done = 0; s->wlen = 0; s->crc = 0; s->memberBytes = 0; s->produced = 0; s->outCap = outCap; s->status = 0; s->errOff = 0;
  for (i = 0 ; i < 8 ; ++i) s->diag[i] = 0;
}
static inline int mgzFail (MgzStream *s, uint32_t status, uint64_t off) { s->status = status; s->errOff = off; s->done = 1; return -1; }

/* One step: a member's header if one is due, then one batch, then the trailer if the batch reached a final block.  0: go on (or s->done); -1: the stream
   is wrong (s->status, s->errOff); -2: the batch could not run (the caller's error) */
static inline int mgzNext (MgzStream *s, MgzPeekFn peek, MgzBatchFn batch, void *ctx)
{
  MgzPlan P;
  MgzSummary S;
  int first = 0;
  if (s->done) return 0;
  if (!s->inMember)
    { uint8_t head[4096];
      const uint64_t at = s->pos >> 3;
      uint64_t len = 0, got;
      int bc, rc;
      if (at >= s->n) { if (!s->diag[MGZ_D_MEMBER]) return mgzFail (s, MGZ_HEADER, at); s->done = 1; return 0; }
      got = peek (ctx, at, head, sizeof (head));
      rc = mgzHeader (head, got, &len, &bc);
      if (rc == 1 && got == sizeof (head))                /* a long extra field, name or comment: walk it in pieces (a header CRC behind them is not checked) */
        { uint32_t flg = head[3], part;
          uint64_t q = at + 10;
          rc = 0;
          if (flg & 4) { if (peek (ctx, q, head, 2) < 2) rc = 1; else q += 2 + ((uint64_t) head[0] | ((uint64_t) head[1] << 8)); }
          for (part = 8 ; part <= 16 && !rc ; part <<= 1)
            if (flg & part)
              for (;;)
                { uint32_t g = peek (ctx, q, head, sizeof (head)), i;
                  if (!g) { rc = 1; break; }
                  for (i = 0 ; i < g && head[i] ; ++i) ;
                  q += i;
                  if (i < g) { ++q; break; }
                }
          if (flg & 2) q += 2;
          if (!rc && q > s->n) rc = 1;
          len = q - at;
        }
      if (rc) return mgzFail (s, rc == 2 ? MGZ_HEADER : MGI_INPUT, at);
      s->pos = (at + len) * 8; s->inMember = 1; s->wlen = 0; s->crc = 0; s->memberBytes = 0; first = 1;
    }
  P.start = s->pos; P.wlen = s->wlen; P.chunkBytes = s->chunkBytes; P.cap = s->cap; P.first = (uint32_t) first;
  { uint64_t fit = (uint64_t) s->batchChunks * s->baseCap / s->cap, left = (s->n - (s->pos >> 3) + s->chunkBytes - 1) / s->chunkBytes;
    if (fit < 1) fit = 1;
    if (left < 1) left = 1;
    P.nChunks = (uint32_t) (fit < left ? fit : left);
  }
  P.outCap = s->outCap - s->produced;
  if (batch (ctx, &P, &S)) { s->done = 1; return -2; }
  ++s->diag[MGZ_D_BATCH]; s->diag[MGZ_D_LAUNCH] += MGZ_LAUNCHES;
  s->diag[MGZ_D_CONF] += S.confirmed; s->diag[MGZ_D_DISC] += S.discarded; s->diag[MGZ_D_FOLD] += S.folded;
  s->diag[MGZ_D_SPEC] += S.confirmed + S.discarded + S.folded;
  if (S.badMarker != MGZ_NONE) return mgzFail (s, MGI_DISTANCE, S.badMarker >> 3);
  s->crc = mgzCrcAppend (s->crc, (uint32_t) S.crc, (uint32_t) S.outBytes);
  s->memberBytes += S.outBytes; s->produced += S.outBytes; s->wlen = (uint32_t) S.wlenAfter; s->pos = S.next;
  if (S.reason == MGZ_ERROR) return mgzFail (s, (uint32_t) S.status, S.errBit >> 3);
  if (S.reason == MGZ_RETRY)
    { ++s->diag[MGZ_D_RETRY];
      if (s->cap >= MGZ_SYM_MAX) return mgzFail (s, MGZ_CAPACITY, S.next >> 3);
      s->cap = s->cap > MGZ_SYM_MAX / 2 ? MGZ_SYM_MAX : s->cap * 2;
      return 0;
    }
  if (s->cap / 2 >= s->baseCap) s->cap /= 2;              /* a batch without an overflow: back towards the guess */
  else s->cap = s->baseCap;
  if (S.reason == MGZ_FINAL)
    { uint8_t t[8];
      const uint64_t at = (S.next + 7) >> 3;
      if (peek (ctx, at, t, 8) < 8) return mgzFail (s, MGI_INPUT, at);
      if (((uint32_t) t[0] | ((uint32_t) t[1] << 8) | ((uint32_t) t[2] << 16) | ((uint32_t) t[3] << 24)) != s->crc) return mgzFail (s, MGI_CRC, at);
      if (((uint32_t) t[4] | ((uint32_t) t[5] << 8) | ((uint32_t) t[6] << 16) | ((uint32_t) t[7] << 24)) != (uint32_t) s->memberBytes) return mgzFail (s, MGI_OUTPUT, at + 4);
      ++s->diag[MGZ_D_MEMBER];
      s->inMember = 0; s->pos = (at + 8) * 8;
      if (at + 8 >= s->n) s->done = 1;
    }
  return 0;
}

/* ---------------------------------------------------------------------------------------------------------------- a batch on one host thread */
/* the caller's memory: nChunks records, nChunks * cap symbols, (nChunks + 1) windows of 32 KiB (slot 0 holds the window the batch starts with and gets the
   one it ends with), the text's room */
typedef struct { const uint8_t *comp; uint64_t n; MgzChunk *ch; uint16_t *sym; uint8_t *win; uint8_t *out; MgInfTables *T; } MgzHostMem;

static inline void mgzBatchHost (const MgzHostMem *M, const MgzPlan *P, MgzSummary *S)
{
  uint32_t c, j;
  uint64_t lo, hi, batchEnd;
  mgzChunkRange (P->start, P->chunkBytes, P->nChunks - 1, M->n, &lo, &batchEnd);
  for (c = 0 ; c < P->nChunks ; ++c)                     /* find */
    { MgzChunk *k = M->ch + c;
      k->cand = P->start; k->end = 0; k->off = 0; k->nSym = 0; k->status = 0; k->final = 0; k->ok = 0; k->wlen = 0; k->pad = 0;
      if (c) { mgzChunkRange (P->start, P->chunkBytes, c, M->n, &lo, &hi); k->cand = mgzFindSerial (M->comp, M->n, lo, hi, M->T); }
    }
  for (c = 0 ; c < P->nChunks ; ++c)                     /* decode */
    { MgzChunk *k = M->ch + c;
      if (k->cand == MGZ_NONE) continue;
      k->status = mgzChunkDecode (M->comp, M->n, k->cand, mgzStopOf (M->ch, P->nChunks, c, batchEnd), c ? ~(uint32_t) 0 : P->wlen,
                                  M->sym + (size_t) c * P->cap, P->cap, M->T, &k->end, &k->nSym, &k->final);
    }
  mgzChainBegin (S, P->start, P->wlen);                  /* chain and windows */
  for (c = 0 ; c < P->nChunks ; )
    { const uint32_t nx = mgzChainStep (M->ch, P->nChunks, c, P->outCap, S);
      if (M->ch[c].ok)
        { const uint8_t *before = M->win + (size_t) c * MGZ_WINDOW;
          uint8_t *after = M->win + (size_t) S->carrySlot * MGZ_WINDOW;
          for (j = 0 ; j < MGZ_WINDOW ; ++j) after[j] = mgzWindowSym (before, M->sym + (size_t) c * P->cap, M->ch[c].nSym, j);
        }
      c = nx;
    }
  mgInfCrcTable (M->T->crcTab, 0, 1);                    /* resolve */
  for (c = 0 ; c < P->nChunks ; ++c)
    { const MgzChunk *k = M->ch + c;
      uint32_t bad = 0, crc;
      if (!k->ok) continue;
      crc = mgzResolveSlice (M->T->crcTab, M->sym + (size_t) c * P->cap, M->win + (size_t) c * MGZ_WINDOW, k->wlen, 0, k->nSym, M->out + k->off, &bad);
      S->crc ^= mgiMulModP (mgiXPow8 ((uint32_t) (S->outBytes - k->off - k->nSym)), crc);
      if (bad && k->cand < S->badMarker) S->badMarker = k->cand;
    }
  if (S->carrySlot) for (j = 0 ; j < MGZ_WINDOW ; ++j) M->win[j] = M->win[(size_t) S->carrySlot * MGZ_WINDOW + j];
}
#endif
