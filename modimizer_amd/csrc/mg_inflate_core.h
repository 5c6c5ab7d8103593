/* mg_inflate_core.h — a raw-deflate (RFC 1951) decoder for ONE gzip member of at most 64 KiB, written once for host and device.
 *
 * No zlib, no allocation, plain C that is also C++ / HIP: mg_inflate.hip compiles it for gfx950 (one lane of a wave decodes, the wave
 * checks the CRC) and for the host (mgInflateMemberHost, the test hook); tools/inflate_host_check.c includes nothing else.
 *
 * BOUNDS.  The decoder reads comp[0 .. cLen) and writes out[0 .. uLen) and touches no other byte of either buffer.  The bit reader
 * CLAMPS: it loads a word of 8 bytes ahead only if the whole word lies below cLen, and single bytes below cLen otherwise (mgiPrime,
 * mgiRefill) -- compressed members are byte-packed, so the words are unaligned loads, and the entry points ask no slack of their callers.  Bits past the input read as absent: whoever needs them gets
 * MGI_INPUT.  A match is copied only after distance <= bytes produced and produced + length <= uLen have been tested.
 *
 * What zlib (inflate with windowBits -15, one member from an empty window) accepts is accepted, what it refuses is refused:
 *   - a Huffman code that is over-subscribed is refused; an incomplete one too, unless it is the single code of length 1 that
 *     inftrees.c lets through for literal/length and distance codes (never for the code-length code); a distance code without any
 *     code is fine until a distance is asked of it;
 *   - HLIT > 29 (more than 286 literal/length codes), HDIST > 29, no end-of-block code, a repeat 16 with no length before it, a
 *     repeat that overruns HLIT + HDIST: MGI_LENGTHS.  A 16 repeats across the literal/length - distance boundary;
 *   - literal/length symbols 286 / 287, distance symbols 30 / 31 and any code word an incomplete code leaves unused: MGI_SYMBOL.
 */
#ifndef MG_INFLATE_CORE_H
#define MG_INFLATE_CORE_H
#include <stdint.h>
#if defined (__HIPCC__)
#define MGI_HD __host__ __device__ static inline
#else
#define MGI_HD static inline
#endif

enum { MGI_OK = 0,
       MGI_INPUT = 1,        /* input exhausted */
       MGI_BLOCKTYPE = 2,    /* block type 3 */
       MGI_STORED = 3,       /* stored LEN / NLEN mismatch */
       MGI_LENGTHS = 4,      /* bad code lengths */
       MGI_SYMBOL = 5,       /* invalid symbol */
       MGI_DISTANCE = 6,     /* distance beyond the start of the member's output */
       MGI_OUTPUT = 7,       /* output longer or shorter than stated */
       MGI_CRC = 8 };        /* CRC-32 mismatch */

/* statistics (optional): what a member reached */
enum { MGI_ST_STORED = 0, MGI_ST_FIXED = 1, MGI_ST_DYNAMIC = 2,   /* deflate blocks by type */
       MGI_ST_LITBITS = 3,                                        /* longest literal/length code of a code that was built */
       MGI_ST_DIST = 4, MGI_ST_MATCH = 5,                         /* longest distance, longest match */
       MGI_ST_DISTBITS = 6,                                       /* longest distance code */
       MGI_ST_SYMBOLS = 7 };                                      /* literal/length symbols decoded */

/* The decode tables of one member: 4608 bytes.  On the device they are the wave's LDS (mg_inflate.hip: one wave a workgroup, so
   160 KiB a CU hold 35 of them, more than the 32 waves a CU runs: LDS does not limit occupancy).
   A `fast` entry is (symbol << 4) | code length for every value of the next LBITS / DBITS input bits that begins with a code of at
   most that many bits, 0 elsewhere: longer codes (and the unused words of an incomplete code) go through the canonical walk over
   `count` and `sym` (codes per length; symbols in code order). */
#define MGI_LBITS 10
#define MGI_DBITS 8
#define MGI_LANES 64         /* slices the CRC is computed in: the lanes of a wave */
typedef struct {
  uint32_t crcTab[256];                     /* 1024: CRC-32 of every byte value (mgInfCrcTable) */
  uint16_t lfast[1 << MGI_LBITS];           /* 2048 */
  uint16_t dfast[1 << MGI_DBITS];           /*  512: the code-length code's first, then the distance code's */
  uint16_t lsym[288], dsym[32];             /*  640 */
  uint16_t lcount[16], dcount[16];          /*   64 */
  uint8_t  lens[320];                       /*  320: code lengths, literal/length then distance */
} MgInfTables;

/* buf: cnt bits, the bytes in[pos - cnt / 8 .. pos).  ahead: the 8 bytes in[apos .. apos + 8), loaded when the word before it was begun, so
   that the load's latency passes behind the symbols decoded meanwhile (ahave: it is there; a word is loaded only if all of it lies below n) */
typedef struct { const uint8_t *in; uint32_t n, pos, cnt, apos, ahave; uint64_t buf, ahead; } MgInfBits;

/* The reader's only loads: a whole 8-byte word (unaligned, little-endian: x86-64 and gfx950) that lies below n, or single bytes below n */
MGI_HD void mgiPrime (MgInfBits *b)
{
  b->apos = b->pos; b->ahave = b->n - b->pos >= 8;
  if (b->ahave) __builtin_memcpy (&b->ahead, b->in + b->pos, 8);
}
MGI_HD void mgiRefill (MgInfBits *b)                      /* at least 32 bits in buf afterwards, or all that is left */
{
  if (b->cnt <= 32 && b->ahave)
    { const uint32_t half = b->pos - b->apos;             /* 0 or 4 */
      b->buf |= (uint64_t) (uint32_t) (b->ahead >> (8 * half)) << b->cnt; b->cnt += 32; b->pos += 4;
      if (half) mgiPrime (b);
      return;
    }
  while (b->cnt <= 56 && b->pos < b->n) { b->buf |= (uint64_t) b->in[b->pos++] << b->cnt; b->cnt += 8; }
}
/* the next k <= 16 bits; 0 if the input does not hold them */
MGI_HD int mgiBits (MgInfBits *b, uint32_t k, uint32_t *v)
{
  if (b->cnt < k) { mgiRefill (b); if (b->cnt < k) return 0; }
  *v = (uint32_t) (b->buf & (((uint64_t) 1 << k) - 1));
  b->buf >>= k; b->cnt -= k;
  return 1;
}

/* The canonical code of n lengths: count, sym and the fast table of fastBits bits.  Returns -1 over-subscribed, else what is left of
   the code space at 15 bits (0: complete); *maxLen is the longest code, 0 if there is none. */
MGI_HD int mgiBuild (const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym, uint16_t *fast, uint32_t fastBits, uint32_t *maxLen)
{
  uint16_t offs[16];
  uint32_t i, len;
  int left = 1;
  for (len = 0 ; len < 16 ; ++len) count[len] = 0;
  for (i = 0 ; i < n ; ++i) ++count[lens[i]];
  for (i = 0 ; i < ((uint32_t) 1 << fastBits) ; ++i) fast[i] = 0;
  *maxLen = 0;
  for (len = 1 ; len < 16 ; ++len)
    { left <<= 1; left -= (int) count[len];
      if (left < 0) return -1;
      if (count[len]) *maxLen = len;
    }
  offs[1] = 0;
  for (len = 1 ; len < 15 ; ++len) offs[len + 1] = (uint16_t) (offs[len] + count[len]);
  for (i = 0 ; i < n ; ++i) if (lens[i]) sym[offs[lens[i]]++] = (uint16_t) i;
  { uint32_t code = 0, idx = 0;
    for (len = 1 ; len <= fastBits ; ++len)
      { uint32_t j;
        for (j = 0 ; j < count[len] ; ++j)
          { const uint32_t c = code + j, s = sym[idx++];
            uint32_t rev = 0, k;
            for (k = 0 ; k < len ; ++k) rev |= ((c >> k) & 1) << (len - 1 - k);
            for (k = rev ; k < ((uint32_t) 1 << fastBits) ; k += (uint32_t) 1 << len) fast[k] = (uint16_t) ((s << 4) | len);
          }
        code = (code + count[len]) << 1;
      }
  }
  return left;
}

/* the next symbol of a code; -1: a code word the code does not have, -2: the input ends inside it */
MGI_HD int mgiDecode (MgInfBits *b, const uint16_t *fast, uint32_t fastBits, const uint16_t *count, const uint16_t *sym)
{
  uint32_t e, len;
  if (b->cnt < 15) mgiRefill (b);
  e = fast[b->buf & (((uint32_t) 1 << fastBits) - 1)];
  len = e & 15;
  if (len)
    { if (len > b->cnt) return -2;
      b->buf >>= len; b->cnt -= len;
      return (int) (e >> 4);
    }
  { int code = 0, first = 0, index = 0;
    uint64_t bits = b->buf;
    for (len = 1 ; len <= 15 ; ++len)
      { int c;
        if (len > b->cnt) return -2;
        code |= (int) (bits & 1); bits >>= 1;
        c = (int) count[len];
        if (code - c < first) { b->buf >>= len; b->cnt -= len; return (int) sym[index + (code - first)]; }
        index += c; first += c; first <<= 1; code <<= 1;
      }
  }
  return -1;
}

#define MGI_STAT_ADD(k) do { if (stats) ++stats[k]; } while (0)
#define MGI_STAT_MAX(k, v) do { if (stats && stats[k] < (uint64_t) (v)) stats[k] = (uint64_t) (v); } while (0)

/* the literal/length and distance codes of a block into T; a status */
MGI_HD uint32_t mgiBlockCodes (MgInfBits *b, uint32_t type, MgInfTables *T, uint64_t *stats)
{
  uint32_t nlen, ndist, i, maxLen = 0;
  int left;
  if (type == 1)
    { for (i = 0 ; i < 144 ; ++i) T->lens[i] = 8;
      for ( ; i < 256 ; ++i) T->lens[i] = 9;
      for ( ; i < 280 ; ++i) T->lens[i] = 7;
      for ( ; i < 288 ; ++i) T->lens[i] = 8;
      for ( ; i < 320 ; ++i) T->lens[i] = 5;
      nlen = 288; ndist = 32;
    }
  else
    { uint32_t ncode, v, total, idx = 0;
      if (!mgiBits (b, 5, &nlen) || !mgiBits (b, 5, &ndist) || !mgiBits (b, 4, &ncode)) return MGI_INPUT;
      nlen += 257; ndist += 1; ncode += 4;
      if (nlen > 286 || ndist > 30) return MGI_LENGTHS;
      for (i = 0 ; i < 19 ; ++i) T->lens[i] = 0;
      for (i = 0 ; i < ncode ; ++i)
        { /* the order the code-length code's lengths come in (RFC 1951 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 */
          const uint32_t at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1);
          if (!mgiBits (b, 3, &v)) return MGI_INPUT;
          T->lens[at] = (uint8_t) v;
        }
      left = mgiBuild (T->lens, 19, T->dcount, T->dsym, T->dfast, MGI_DBITS, &maxLen);
      if (left) return MGI_LENGTHS;                      /* over-subscribed, or incomplete: never accepted for this code */
      total = nlen + ndist;
      while (idx < total)
        { const int s = mgiDecode (b, T->dfast, MGI_DBITS, T->dcount, T->dsym);
          uint32_t rep, val = 0;
          if (s < 0) return s == -2 ? MGI_INPUT : MGI_LENGTHS;
          if (s < 16) { T->lens[idx++] = (uint8_t) s; continue; }
          if (s == 16)
            { if (!idx) return MGI_LENGTHS;                /* nothing to repeat */
              val = T->lens[idx - 1];
              if (!mgiBits (b, 2, &rep)) return MGI_INPUT;
              rep += 3;
            }
          else if (s == 17) { if (!mgiBits (b, 3, &rep)) return MGI_INPUT; rep += 3; }
          else { if (!mgiBits (b, 7, &rep)) return MGI_INPUT; rep += 11; }
          if (idx + rep > total) return MGI_LENGTHS;       /* the run leaves HLIT + HDIST */
          while (rep--) T->lens[idx++] = (uint8_t) val;
        }
      if (!T->lens[256]) return MGI_LENGTHS;               /* no end-of-block code */
    }
  left = mgiBuild (T->lens, nlen, T->lcount, T->lsym, T->lfast, MGI_LBITS, &maxLen);
  if (left < 0 || (left > 0 && maxLen != 1)) return MGI_LENGTHS;
  MGI_STAT_MAX (MGI_ST_LITBITS, maxLen);
  left = mgiBuild (T->lens + nlen, ndist, T->dcount, T->dsym, T->dfast, MGI_DBITS, &maxLen);
  if (left < 0 || (left > 0 && maxLen > 1)) return MGI_LENGTHS;      /* (no distance code at all is fine: literals only) */
  MGI_STAT_MAX (MGI_ST_DISTBITS, maxLen);
  return MGI_OK;
}

/* A stored block's header (RFC 1951 3.2.4): to the byte boundary, LEN and its complement, and the whole bytes that were loaded ahead go back, so that the
   reader holds no bits and in[pos] is the first payload byte.  Returns LEN, which the input holds -- the caller copies the bytes, moves pos past them and
   primes the reader again -- or minus a status */
MGI_HD int mgiStoredHeader (MgInfBits *b)
{
  uint32_t len, nlen;
  b->buf >>= b->cnt & 7; b->cnt -= b->cnt & 7;
  if (!mgiBits (b, 16, &len) || !mgiBits (b, 16, &nlen)) return -MGI_INPUT;
  if ((len ^ 0xffffu) != nlen) return -MGI_STORED;
  b->pos -= b->cnt >> 3; b->cnt = 0; b->buf = 0; b->ahave = 0;
  return len > b->n - b->pos ? -MGI_INPUT : (int) len;
}

/* A match (RFC 1951 3.2.5), in two steps.  mgiLength: the literal/length symbol s > 256 that was just decoded and its extra bits into *len (3 .. 258);
   mgiDistance: the distance symbol behind it and its extra bits into *dist (1 .. 32768).  A status each; whether they fit is the caller's to say */
MGI_HD uint32_t mgiLength (MgInfBits *b, int s, uint32_t *len)
{
  uint32_t extra, v = 0;
  if (s > 285) return MGI_SYMBOL;
  /* 257 .. 264 no extra bits, then four codes to each number of extra bits, 285 is 258 */
  if (s < 265) { *len = (uint32_t) s - 254; return MGI_OK; }
  if (s == 285) { *len = 258; return MGI_OK; }
  extra = ((uint32_t) s - 261) >> 2; *len = 3 + ((4 + (((uint32_t) s - 261) & 3)) << extra);
  if (!mgiBits (b, extra, &v)) return MGI_INPUT;
  *len += v;
  return MGI_OK;
}
MGI_HD uint32_t mgiDistance (MgInfBits *b, const MgInfTables *T, uint32_t *dist)
{
  uint32_t extra, v = 0;
  const int s = mgiDecode (b, T->dfast, MGI_DBITS, T->dcount, T->dsym);
  if (s < 0) return s == -2 ? MGI_INPUT : MGI_SYMBOL;
  if (s > 29) return MGI_SYMBOL;
  /* 0 .. 3 no extra bits, then two codes to each number of extra bits */
  if (s < 4) { *dist = (uint32_t) s + 1; return MGI_OK; }
  extra = ((uint32_t) s >> 1) - 1; *dist = 1 + ((2 + ((uint32_t) s & 1)) << extra);
  if (!mgiBits (b, extra, &v)) return MGI_INPUT;
  *dist += v;
  return MGI_OK;
}

/* One member: comp[0 .. cLen) inflated into out[0 .. uLen).  Returns MGI_OK .. MGI_OUTPUT; the CRC is the caller's (mgInfCrcSlice).
   stats: 0, or 8 counters that are raised, not cleared. */
MGI_HD uint32_t mgInfInflate (const uint8_t *comp, uint32_t cLen, uint8_t *out, uint32_t uLen, MgInfTables *T, uint64_t *stats)
{
  MgInfBits bits, *b = &bits;
  uint32_t o = 0, last = 0, type = 0;
  b->in = comp; b->n = cLen; b->pos = 0; b->cnt = 0; b->buf = 0; b->ahead = 0;
  mgiPrime (b);
  do
    { if (!mgiBits (b, 1, &last) || !mgiBits (b, 2, &type)) return MGI_INPUT;
      if (type == 3) return MGI_BLOCKTYPE;
      if (type == 0)
        { uint32_t len, i;
          MGI_STAT_ADD (MGI_ST_STORED);
          { const int h = mgiStoredHeader (b); if (h < 0) return (uint32_t) -h; len = (uint32_t) h; }
          if (len > uLen - o) return MGI_OUTPUT;
          for (i = 0 ; i < len ; ++i) out[o + i] = b->in[b->pos + i];
          o += len; b->pos += len;
          mgiPrime (b);
          continue;
        }
      MGI_STAT_ADD (type == 1 ? MGI_ST_FIXED : MGI_ST_DYNAMIC);
      { const uint32_t st = mgiBlockCodes (b, type, T, stats); if (st) return st; }
      for (;;)
        { int s = mgiDecode (b, T->lfast, MGI_LBITS, T->lcount, T->lsym);
          uint32_t len, dist, i;
          if (s < 0) return s == -2 ? MGI_INPUT : MGI_SYMBOL;
          MGI_STAT_ADD (MGI_ST_SYMBOLS);
          if (s < 256) { if (o >= uLen) return MGI_OUTPUT; out[o++] = (uint8_t) s; continue; }
          if (s == 256) break;
          { uint32_t st = mgiLength (b, s, &len); if (!st) st = mgiDistance (b, T, &dist); if (st) return st; }
          if (dist > o) return MGI_DISTANCE;
          if (len > uLen - o) return MGI_OUTPUT;
          MGI_STAT_MAX (MGI_ST_DIST, dist); MGI_STAT_MAX (MGI_ST_MATCH, len);
          /* the copy: this thread reads what it wrote itself, in program order.  From distance 8 up in words of 8 bytes -- a word read
             ends at or before the byte being written, so it holds bytes that exist, also where dist < len repeats what this copy wrote --
             and exactly len bytes are stored; below 8 byte by byte */
          if (dist >= 8)
            { uint64_t v;
              for (i = 0 ; i + 8 <= len ; i += 8) { __builtin_memcpy (&v, out + o + i - dist, 8); __builtin_memcpy (out + o + i, &v, 8); }
              if (i < len)
                { __builtin_memcpy (&v, out + o + i - dist, 8);
                  for ( ; i < len ; ++i, v >>= 8) out[o + i] = (uint8_t) v;
                }
            }
          else for (i = 0 ; i < len ; ++i) out[o + i] = out[o + i - dist];
          o += len;
        }
    }
  while (!last);
  return o == uLen ? MGI_OK : MGI_OUTPUT;
}

/* ---- CRC-32 (the gzip polynomial, reflected: 0xedb88320) in slices ----
 * crc (A B) = crc (A) x^(8 |B|) + crc (B) in GF(2)[x] mod the polynomial, for the finished CRCs zlib's crc32 () returns: the
 * arithmetic of its crc32_combine.  So the CRC of a text cut into slices is the sum (xor) over the slices of their own CRC times
 * x^(8 * bytes after the slice): every lane takes a slice, the wave xors. */
#define MGI_POLY 0xedb88320u
MGI_HD void mgInfCrcTable (uint32_t *tab, uint32_t lane, uint32_t nLanes)      /* entries lane, lane + nLanes .. */
{
  uint32_t i, k;
  for (i = lane ; i < 256 ; i += nLanes)
    { uint32_t c = i;
      for (k = 0 ; k < 8 ; ++k) c = (c & 1) ? (c >> 1) ^ MGI_POLY : c >> 1;
      tab[i] = c;
    }
}
MGI_HD uint32_t mgiMulModP (uint32_t a, uint32_t b)      /* a(x) b(x) mod p(x), bit 31 is x^0 */
{
  uint32_t m = (uint32_t) 1 << 31, p = 0;
  if (!a) return 0;
  for (;;)
    { if (a & m) { p ^= b; if (!(a & (m - 1))) break; }
      m >>= 1;
      b = (b & 1) ? (b >> 1) ^ MGI_POLY : b >> 1;
    }
  return p;
}
MGI_HD uint32_t mgiXPow8 (uint32_t nBytes)                /* x^(8 nBytes) mod p(x) */
{
  uint32_t p = (uint32_t) 1 << 31, sq = (uint32_t) 1 << 23;      /* x^0; x^8 */
  while (nBytes)
    { if (nBytes & 1) p = mgiMulModP (sq, p);
      nBytes >>= 1;
      if (nBytes) sq = mgiMulModP (sq, sq);
    }
  return p;
}
/* this lane's share of the CRC-32 of out[0 .. uLen): the xor over lane = 0 .. MGI_LANES - 1 is the CRC */
MGI_HD uint32_t mgInfCrcSlice (const uint32_t *tab, const uint8_t *out, uint32_t uLen, uint32_t lane)
{
  const uint32_t per = (uLen + MGI_LANES - 1) / MGI_LANES;
  const uint32_t a = lane * per < uLen ? lane * per : uLen, e = a + per < uLen ? a + per : uLen;
  uint32_t c = 0xffffffffu, i;
  if (a == e) return 0;
  for (i = a ; i < e ; ++i) c = tab[(c ^ out[i]) & 0xff] ^ (c >> 8);
  c ^= 0xffffffffu;
  return e == uLen ? c : mgiMulModP (mgiXPow8 (uLen - e), c);
}

/* the whole of it on one thread: inflate, then the slices' CRCs in turn.  What mgInflateMemberHost and the sanitizer program run. */
MGI_HD uint32_t mgInfMember (const uint8_t *comp, uint32_t cLen, uint8_t *out, uint32_t uLen, uint32_t crc, MgInfTables *T, uint64_t *stats)
{
  uint32_t st, lane, c = 0;
  st = mgInfInflate (comp, cLen, out, uLen, T, stats);
  if (st) return st;
  mgInfCrcTable (T->crcTab, 0, 1);
  for (lane = 0 ; lane < MGI_LANES ; ++lane) c ^= mgInfCrcSlice (T->crcTab, out, uLen, lane);
  return c == crc ? MGI_OK : MGI_CRC;
}
#endif
