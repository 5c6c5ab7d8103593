/* mg_deflate_core.h — a raw-deflate (RFC 1951) ENCODER for ONE block of at most 65280 text bytes, written once for host and device: the block
 * becomes one complete BGZF member (RFC 1952 with the 'BC' extra field) of at most 65536 bytes.  The mirror of mg_inflate_core.h: no zlib, no
 * allocation, plain C that is also C++ / HIP.  mg_deflate.hip compiles it for gfx950 (one workgroup a block) and for the host
 * (mgDeflateBlockHost, the test hook); tools/deflate_host_check.c includes nothing but the two core headers.
 *
 * ONE FUNCTION, ANY NUMBER OF LANES.  mgDefMember is called by every lane of a team with (lane, nLanes): the kernel's 256 threads, or one host
 * thread as lane 0 of 1.  Phases that are parallel are loops strided by nLanes; phases that are serial run on lane 0; MGD_SYNC () -- the
 * workgroup barrier on the device, nothing on the host -- stands between them, always in uniform control flow.  The member is a pure function
 * of the block's bytes, whatever nLanes is:
 *
 *   MATCHING.  LZ77 over a table head[hash of the next 4 bytes] of the latest earlier position, one candidate, no chains.  The text is taken
 * in steps of MGD_STEP positions.  A position's candidate is the table's state at the START of its step; after the lookups of a step each
 * bucket is raised to the largest position of the step that hashes to it (positions are stored + 1, so "latest" is "max": an LDS atomicMax
 * on the device, a plain loop on the host, the same table either way).  The second candidate of every position is the byte before it
 * (distance 1: runs).  The longer of the two counts, distance 1 on a tie; lengths 3 .. 258, distances 1 .. 32768, never before the block's
 * first byte.  A match is kept only if it is likely to be cheaper than its literals: 3 * length >= 13 + the distance's extra bits.
 *   Overlaps are resolved greedily in text order, step by step, out of the step's results in the work area (LDS on the device).  The walk is
 * serial and has one result; it is the one phase written twice: a plain loop on lane 0 for the host, and for the device the first wave
 * taking 64 positions into its lanes and walking them with lane reads, so that no memory access lies on the serial chain.
 *
 *   CODING.  From its own histograms the encoder computes the EXACT bit cost of (a) a stored block, (b) a dynamic-Huffman block of literals
 * only, (c) a dynamic-Huffman block with the matches, and writes the cheapest ((a) before (b) before (c) on a tie); (b) and (c) are also
 * priced with the fixed code, which wins for texts of a few bytes (what zlib does with them, and what the tests hold the sizes against).  Code lengths: the
 * symbols in use sorted by (count, symbol) -- a rank sort, every lane ranks its share -- Moffat and Katajainen's in-place minimum-redundancy
 * lengths, the Kraft sum repaired to the limit (15 bits; 7 for the code-length code) by moving the deepest codes up, and the lengths handed
 * out longest first to the rarest symbols.  A code with fewer than two symbols in use gets dummies, as zlib's encoder does, so every code
 * written is complete.  The lengths are run-length coded with 16 / 17 / 18 over literal/length and distance lengths as one row.
 *
 *   EMISSION.  The exact cost is also the layout: the member's length is known before a bit is written, every token's bit offset is a prefix
 * sum, and every lane writes the bits of its contiguous share of the tokens.  The slot is a row of 32-bit words that are zeroed first; a
 * word that a lane's share covers entirely is stored, a word it covers in part is OR-ed (atomicOr on the device) -- every lane that touches
 * such a word covers it in part, so no word sees both kinds of access.  Header and trailer bytes are OR-ed in the same way.
 *
 * BOUNDS.  Reads stay inside text[0 .. uLen) and tokens[0 .. uLen); every store to the slot is tested against its 65536 bytes (16384 words);
 * every loop is bounded by uLen or by a table's size.  No slack is asked of any buffer.  On the device the slot is 4-byte aligned. */
#ifndef MG_DEFLATE_CORE_H
#define MG_DEFLATE_CORE_H
#include <stdint.h>
#include "mg_inflate_core.h"                             /* MGI_HD, the CRC-32 in slices */

#define MGD_BLOCK_MAX 65280u                             /* text bytes of a block: bgzip's */
#define MGD_SLOT      65536u                             /* bytes of a member, at most */
#define MGD_HASH_BITS 12
#define MGD_STEP      1024u                              /* positions whose candidates are looked up before any of them enters the table */
#define MGD_MAX_LANES 256u
#define MGD_MATCH     0x80000000u                        /* a token: a literal's byte, or this | length << 16 | distance - 1 */

#if defined (__HIP_DEVICE_COMPILE__)
#define MGD_SYNC() __syncthreads ()
#define MGD_ADD(p, v) ((void) atomicAdd ((p), (v)))
#define MGD_MAX(p, v) ((void) atomicMax ((p), (v)))
#else
#define MGD_SYNC() ((void) 0)
#define MGD_ADD(p, v) ((void) (*(p) += (v)))
#define MGD_MAX(p, v) ((void) (*(p) < (v) ? (*(p) = (v)) : 0u))
#endif

enum { MGD_ST_KIND = 0,                                  /* 0 stored, 1 literals only, 2 with matches */
       MGD_ST_LITERALS = 1, MGD_ST_MATCHES = 2,          /* of the block as written */
       MGD_ST_MATCH = 3, MGD_ST_DIST = 4,                /* longest match, longest distance */
       MGD_ST_LITBITS = 5, MGD_ST_DISTBITS = 6,          /* longest literal/length code, longest distance code */
       MGD_ST_BITS = 7 };                                /* bits of the deflate payload */

/* one dynamic block's code: lengths, the run-length coded header, the exact size */
typedef struct {
  uint8_t  litLen[288], distLen[32], clLen[19];
  uint16_t rle[320];                                     /* code-length symbol | extra value << 8 */
  uint32_t nRle, hlit, hdist, hclen, maxLit, maxDist;
  uint32_t hdrBits, bits;                                /* the block's bits up to the first token; all of them */
} MgDefCode;

/* the work area of one block: about 30 KiB.  On the device it is the workgroup's LDS (mg_deflate.hip: five of them fit a CU's 160 KiB) */
typedef struct {
  uint32_t head[1u << MGD_HASH_BITS];                    /* 16384: latest position + 1 by hash */
  uint32_t step[MGD_STEP];                               /*  4096: a step's candidates, then its tokens-to-be */
  uint32_t crcTab[256];
  uint32_t freqB[288], freqC[288], distFreq[32], zero[32], clFreq[19];      /* literals only; with matches */
  uint32_t keys[288], sorted[288], count[64], next[16];      /* (the code builders' small tables live here: no private arrays) */
  uint16_t litCode[288], distCode[32], clCode[19];       /* of the code that is written, bit-reversed */
  MgDefCode code[2];                                     /* [0] literals only, [1] with matches */
  uint32_t laneBits[MGD_MAX_LANES];
  uint32_t crcPart[MGI_LANES];
  uint32_t nTok, nMatch, maxMatch, maxDist, extraBits, kind, fixed, memberLen, m;
} MgDefWork;

/* ---- the slot as words ---- */
MGI_HD void mgdWordSet (uint8_t *out, uint32_t w, uint32_t v)
{
  if (w >= MGD_SLOT / 4) return;
#if defined (__HIP_DEVICE_COMPILE__)
  ((uint32_t *) out)[w] = v;
#else
  __builtin_memcpy (out + 4 * w, &v, 4);
#endif
}
MGI_HD void mgdWordOr (uint8_t *out, uint32_t w, uint32_t v)
{
  if (w >= MGD_SLOT / 4) return;
#if defined (__HIP_DEVICE_COMPILE__)
  (void) atomicOr ((unsigned int *) out + w, v);
#else
  { uint32_t o; __builtin_memcpy (&o, out + 4 * w, 4); o |= v; __builtin_memcpy (out + 4 * w, &o, 4); }
#endif
}
MGI_HD void mgdBytesOr (uint8_t *out, uint32_t at, uint64_t v, uint32_t n)      /* n <= 8 bytes of v, little-endian, at byte `at` */
{
  uint32_t i;
  for (i = 0 ; i < n ; ++i) mgdWordOr (out, (at + i) >> 2, (uint32_t) ((v >> (8 * i)) & 0xff) << (8 * ((at + i) & 3)));
}

/* bits into the slot from bit `bit` on: whole words are stored, the first and the last word of the range are OR-ed where others share them */
typedef struct { uint8_t *out; uint64_t acc; uint32_t n, w; int shared; } MgdPut;
MGI_HD void mgdPutStart (MgdPut *e, uint8_t *out, uint32_t bit) { e->out = out; e->acc = 0; e->n = bit & 31; e->w = bit >> 5; e->shared = (bit & 31) != 0; }
MGI_HD void mgdPut (MgdPut *e, uint32_t v, uint32_t k)    /* k <= 28 */
{
  e->acc |= (uint64_t) v << e->n; e->n += k;
  if (e->n >= 32)
    { if (e->shared) mgdWordOr (e->out, e->w, (uint32_t) e->acc); else mgdWordSet (e->out, e->w, (uint32_t) e->acc);
      e->shared = 0; ++e->w; e->acc >>= 32; e->n -= 32;
    }
}
MGI_HD void mgdPutEnd (MgdPut *e) { if (e->n) mgdWordOr (e->out, e->w, (uint32_t) e->acc); }

/* ---- symbols (RFC 1951 3.2.5) ---- */
MGI_HD uint32_t mgdLog2 (uint32_t v) { return 31u - (uint32_t) __builtin_clz (v); }      /* v > 0 */
MGI_HD void mgdLenSym (uint32_t len, uint32_t *sym, uint32_t *eb, uint32_t *ev)           /* 3 .. 258 */
{
  const uint32_t l = len - 3;
  if (len == 258) { *sym = 285; *eb = 0; *ev = 0; }
  else if (l < 8) { *sym = 257 + l; *eb = 0; *ev = 0; }
  else { const uint32_t e = mgdLog2 (l) - 2; *sym = 261 + 4 * e + ((l >> e) & 3); *eb = e; *ev = l & ((1u << e) - 1); }
}
MGI_HD void mgdDistSym (uint32_t dist, uint32_t *sym, uint32_t *eb, uint32_t *ev)         /* 1 .. 32768 */
{
  const uint32_t d = dist - 1;
  if (d < 4) { *sym = d; *eb = 0; *ev = 0; }
  else { const uint32_t k = mgdLog2 (d); *sym = 2 * k + ((d >> (k - 1)) & 1); *eb = k - 1; *ev = d & ((1u << (k - 1)) - 1); }
}

/* ---- matching ---- */
MGI_HD uint32_t mgdHash (const uint8_t *p)
{
  const uint32_t v = (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
  return (v * 2654435761u) >> (32 - MGD_HASH_BITS);
}
MGI_HD uint32_t mgdMatchLen (const uint8_t *text, uint32_t a, uint32_t b, uint32_t maxLen)      /* a < b, b + maxLen <= the block's length */
{
  uint32_t i = 0;
  while (i + 8 <= maxLen)
    { uint64_t x, y;
      __builtin_memcpy (&x, text + a + i, 8); __builtin_memcpy (&y, text + b + i, 8);
      if (x != y) return i + ((uint32_t) __builtin_ctzll (x ^ y) >> 3);
      i += 8;
    }
  while (i < maxLen && text[a + i] == text[b + i]) ++i;
  return i;
}

/* ---- code lengths ---- */

/* lens[0 .. n) for freq[0 .. n): a complete prefix code of at most maxBits over the symbols in use (two at least: dummies are added).  All lanes */
MGI_HD void mgdBuildLens (const uint32_t *freq, uint32_t n, uint32_t maxBits, uint8_t *lens, MgDefWork *W, uint32_t lane, uint32_t nLanes)
{
  uint32_t i;
  if (lane == 0)                                         /* the symbols in use, as keys count << 9 | symbol: all different */
    { uint32_t m = 0;
      for (i = 0 ; i < n ; ++i) { lens[i] = 0; if (freq[i]) W->keys[m++] = (freq[i] << 9) | i; }
      if (m < 2) { const uint32_t d = (m && (W->keys[0] & 511u) == 0) ? 1u : 0u; W->keys[m++] = d; }      /* (count 0) */
      if (m < 2) W->keys[m++] = 1u;                      /* nothing was in use: symbols 0 and 1 */
      W->m = m;
    }
  MGD_SYNC ();
  { const uint32_t m = W->m;
    for (i = lane ; i < m ; i += nLanes)
      { const uint32_t k = W->keys[i]; uint32_t j, r = 0;
        for (j = 0 ; j < m ; ++j) r += W->keys[j] < k;
        W->sorted[r] = k;
      }
  }
  MGD_SYNC ();
  if (lane == 0)
    { const int m = (int) W->m;
      uint32_t *A = W->keys, *count = W->count, total, guard;
      int root, leaf, next, avbl, used, dpth;
      for (i = 0 ; i < (uint32_t) m ; ++i) A[i] = W->sorted[i] >> 9;
      /* Moffat & Katajainen, "In-place calculation of minimum-redundancy codes" (1995): A[] ascending counts in, code lengths out */
      if (m == 2) { A[0] = A[1] = 1; }
      else
        { A[0] += A[1]; root = 0; leaf = 2;
          for (next = 1 ; next < m - 1 ; ++next)
            { if (leaf >= m || A[root] <= A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t) next; } else A[next] = A[leaf++];      /* (a tie: the node, not the leaf) */
              if (leaf >= m || (root < next && A[root] <= A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t) next; } else A[next] += A[leaf++];
            }
          A[m - 2] = 0;
          for (next = m - 3 ; next >= 0 ; --next) A[next] = A[A[next]] + 1;
          avbl = 1; used = dpth = 0; root = m - 2; next = m - 1;
          while (avbl > 0 && dpth < 288)
            { while (root >= 0 && (int) A[root] == dpth) { ++used; --root; }
              while (avbl > used && next >= 0) { A[next--] = (uint32_t) dpth; --avbl; }
              avbl = 2 * used; ++dpth; used = 0;
            }
        }
      /* the lengths' counts, brought under the limit: what is deeper moves to the limit, then the Kraft sum is repaired */
      for (i = 0 ; i < 64 ; ++i) count[i] = 0;
      for (i = 0 ; i < (uint32_t) m ; ++i) { const uint32_t l = A[i] < 1 ? 1 : A[i] > maxBits ? maxBits : A[i]; ++count[l]; }
      total = 0;
      for (i = maxBits ; i > 0 ; --i) total += count[i] << (maxBits - i);
      for (guard = 0 ; total > ((uint32_t) 1 << maxBits) && guard < 1024 ; ++guard)
        { --count[maxBits];
          for (i = maxBits - 1 ; i > 0 ; --i) if (count[i]) { --count[i]; count[i + 1] += 2; break; }
          --total;
        }
      /* longest codes to the rarest symbols */
      { uint32_t at = 0, l, c;
        for (l = maxBits ; l > 0 ; --l)
          for (c = 0 ; c < count[l] && at < (uint32_t) m ; ++c) lens[W->sorted[at++] & 511u] = (uint8_t) l;
      }
    }
  MGD_SYNC ();
}

/* canonical codes of lens[0 .. n), bit-reversed for the writer.  Lane 0 */
MGI_HD void mgdAssignCodes (MgDefWork *W, const uint8_t *lens, uint32_t n, uint16_t *codes)
{
  uint32_t *count = W->count, *next = W->next, i, code = 0;
  for (i = 0 ; i < 16 ; ++i) count[i] = 0;
  for (i = 0 ; i < n ; ++i) ++count[lens[i] & 15];
  count[0] = 0;
  for (i = 1 ; i < 16 ; ++i) { code = (code + count[i - 1]) << 1; next[i] = code; }
  for (i = 0 ; i < n ; ++i)
    { const uint32_t l = lens[i] & 15; uint32_t c, r = 0, k;
      if (!l) { codes[i] = 0; continue; }
      c = next[l]++;
      for (k = 0 ; k < l ; ++k) r |= ((c >> k) & 1) << (l - 1 - k);
      codes[i] = (uint16_t) r;
    }
}

MGI_HD uint32_t mgdClOrder (uint32_t i)                  /* RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 */
{ return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1); }

MGI_HD void mgdRleAdd (MgDefWork *W, MgDefCode *c, uint32_t sym, uint32_t extra)
{ if (c->nRle < 320) { c->rle[c->nRle++] = (uint16_t) (sym | (extra << 8)); ++W->clFreq[sym]; } }

/* the code of a dynamic block from its histograms: lengths, header, exact size.  All lanes */
MGI_HD void mgdMakeCode (MgDefWork *W, MgDefCode *c, const uint32_t *litFreq, const uint32_t *distFreq, uint32_t extraBits, uint32_t lane, uint32_t nLanes)
{
  mgdBuildLens (litFreq, 286, 15, c->litLen, W, lane, nLanes);
  mgdBuildLens (distFreq, 30, 15, c->distLen, W, lane, nLanes);
  if (lane == 0)
    { uint32_t i, total, bits = 0;
      c->hlit = 286; while (c->hlit > 257 && !c->litLen[c->hlit - 1]) --c->hlit;
      c->hdist = 30; while (c->hdist > 1 && !c->distLen[c->hdist - 1]) --c->hdist;
      c->maxLit = c->maxDist = 0;
      for (i = 0 ; i < 286 ; ++i) { if (c->litLen[i] > c->maxLit) c->maxLit = c->litLen[i]; bits += litFreq[i] * c->litLen[i]; }
      for (i = 0 ; i < 30 ; ++i) { if (c->distLen[i] > c->maxDist) c->maxDist = c->distLen[i]; bits += distFreq[i] * c->distLen[i]; }
      c->bits = bits + extraBits;
      for (i = 0 ; i < 19 ; ++i) W->clFreq[i] = 0;
      c->nRle = 0;
      total = c->hlit + c->hdist;
      i = 0;
      while (i < total)
        { const uint32_t v = i < c->hlit ? c->litLen[i] : c->distLen[i - c->hlit];
          uint32_t run = 1;
          while (i + run < total && (i + run < c->hlit ? c->litLen[i + run] : c->distLen[i + run - c->hlit]) == v) ++run;
          i += run;
          if (!v)
            { while (run >= 11) { const uint32_t k = run < 138 ? run : 138; mgdRleAdd (W, c, 18, k - 11); run -= k; }
              if (run >= 3) { mgdRleAdd (W, c, 17, run - 3); run = 0; }
              while (run) { mgdRleAdd (W, c, 0, 0); --run; }
            }
          else
            { mgdRleAdd (W, c, v, 0); --run;
              while (run >= 3) { const uint32_t k = run < 6 ? run : 6; mgdRleAdd (W, c, 16, k - 3); run -= k; }
              while (run) { mgdRleAdd (W, c, v, 0); --run; }
            }
        }
    }
  MGD_SYNC ();
  mgdBuildLens (W->clFreq, 19, 7, c->clLen, W, lane, nLanes);
  if (lane == 0)
    { uint32_t i, hdr;
      c->hclen = 19; while (c->hclen > 4 && !c->clLen[mgdClOrder (c->hclen - 1)]) --c->hclen;
      hdr = 3 + 5 + 5 + 4 + 3 * c->hclen + 2 * W->clFreq[16] + 3 * W->clFreq[17] + 7 * W->clFreq[18];
      for (i = 0 ; i < 19 ; ++i) hdr += W->clFreq[i] * c->clLen[i];
      c->hdrBits = hdr; c->bits += hdr;
    }
  MGD_SYNC ();
}

/* the bits of one item of the block: a token, or behind the last one the end-of-block code */
MGI_HD uint32_t mgdItemBits (const MgDefCode *c, uint32_t t)
{
  uint32_t s, eb, ev, bits;
  if (!(t & MGD_MATCH)) return c->litLen[t & 0x1ffu];
  mgdLenSym ((t >> 16) & 0x1ffu, &s, &eb, &ev); bits = c->litLen[s] + eb;
  mgdDistSym ((t & 0x7fffu) + 1, &s, &eb, &ev);
  return bits + c->distLen[s] + eb;
}
MGI_HD void mgdItemPut (MgdPut *e, const MgDefWork *W, const MgDefCode *c, uint32_t t)
{
  uint32_t s, eb, ev;
  if (!(t & MGD_MATCH)) { mgdPut (e, W->litCode[t & 0x1ffu], c->litLen[t & 0x1ffu]); return; }
  mgdLenSym ((t >> 16) & 0x1ffu, &s, &eb, &ev);
  mgdPut (e, W->litCode[s] | (ev << c->litLen[s]), c->litLen[s] + eb);
  mgdDistSym ((t & 0x7fffu) + 1, &s, &eb, &ev);
  mgdPut (e, W->distCode[s], c->distLen[s]);
  if (eb) mgdPut (e, ev, eb);
}

/* a token that the greedy walk has taken: its symbols into the histograms of the block with matches, its share of the statistics */
MGI_HD void mgdCountToken (MgDefWork *W, uint32_t t)
{
  if (t & MGD_MATCH)
    { const uint32_t len = (t >> 16) & 0x1ffu, dist = (t & 0x7fffu) + 1;
      uint32_t s, eb, ev, extra;
      mgdLenSym (len, &s, &eb, &ev); MGD_ADD (&W->freqC[s], 1u); extra = eb;
      mgdDistSym (dist, &s, &eb, &ev); MGD_ADD (&W->distFreq[s], 1u); extra += eb;
      if (extra) MGD_ADD (&W->extraBits, extra);
      MGD_ADD (&W->nMatch, 1u); MGD_MAX (&W->maxMatch, len); MGD_MAX (&W->maxDist, dist);
    }
  else MGD_ADD (&W->freqC[t & 0xffu], 1u);
}

/* One block: text[0 .. n), n <= 65280, to one BGZF member in out[0 .. 65536).  tokens: n words of the caller's (a slice of device scratch; the host's
   own array), W: the work area, shared by the lanes.  Every lane of the team calls it with the same arguments but `lane`.  Returns the member's
   length (the same on every lane).  stats: 0, or 8 counters that lane 0 sets. */
MGI_HD uint32_t mgDefMember (const uint8_t *text, uint32_t n, uint8_t *out, uint32_t *tokens, MgDefWork *W, uint32_t lane, uint32_t nLanes, uint64_t *stats)
{
  uint32_t i, s0, pos = 0, nTok = 0;                     /* the greedy walk's place and its tokens so far: lane 0's on the host, the first wave's (every lane the same) on the device */
  if (n > MGD_BLOCK_MAX) n = MGD_BLOCK_MAX;
  mgInfCrcTable (W->crcTab, lane, nLanes);
  for (i = lane ; i < (1u << MGD_HASH_BITS) ; i += nLanes) W->head[i] = 0;
  for (i = lane ; i < 288 ; i += nLanes) { W->freqB[i] = 0; W->freqC[i] = 0; }
  for (i = lane ; i < 32 ; i += nLanes) { W->distFreq[i] = 0; W->zero[i] = 0; }
  if (lane == 0) { W->nMatch = 0; W->maxMatch = 0; W->maxDist = 0; W->extraBits = 0; }
  MGD_SYNC ();

  /* ---- matches, step by step ---- */
  for (s0 = 0 ; s0 < n ; s0 += MGD_STEP)
    { const uint32_t s1 = n - s0 < MGD_STEP ? n : s0 + MGD_STEP;
      uint32_t p;
      for (p = s0 + lane ; p < s1 ; p += nLanes) W->step[p - s0] = n - p >= 4 ? W->head[mgdHash (text + p)] : 0;
      MGD_SYNC ();
      for (p = s0 + lane ; p < s1 ; p += nLanes)
        { const uint32_t maxLen = n - p < 258 ? n - p : 258, c = W->step[p - s0], b = text[p];
          uint32_t len = 0, dist = 1, tok = b;
          if (n - p >= 4) MGD_MAX (&W->head[mgdHash (text + p)], p + 1);
          MGD_ADD (&W->freqB[b], 1u);
          if (p) len = mgdMatchLen (text, p - 1, p, maxLen);
          if (c && c <= p && p - (c - 1) <= 32768u)
            { const uint32_t l = mgdMatchLen (text, c - 1, p, maxLen);
              if (l > len) { len = l; dist = p - (c - 1); }
            }
          if (len >= 3)
            { uint32_t s, eb, ev;
              mgdDistSym (dist, &s, &eb, &ev);
              if (3 * len >= 13 + eb) tok = MGD_MATCH | (len << 16) | (dist - 1);
            }
          W->step[p - s0] = tok;
        }
      MGD_SYNC ();
      /* greedy, in text order: a match that is taken hides the positions under it */
#if defined (__HIP_DEVICE_COMPILE__)
      /* The first wave, 64 positions at a time: every lane holds one position's result, the walk over them is scalar -- a lane read and an
         add a token, no memory on the chain -- and marks the tokens' positions in a mask; then the marked lanes store their tokens side by
         side and count them.  The same tokens in the same order as the host's loop below: the greedy walk has one result */
      if (lane < 64)
        { uint32_t base;
          for (base = s0 ; base < s1 ; base += 64)
            { const uint32_t end = s1 - base < 64 ? s1 : base + 64;
              const uint32_t t = base + lane < s1 ? W->step[base + lane - s0] : 0;
              uint64_t starts = 0;
              while (pos < end)
                { const uint32_t at = (uint32_t) __builtin_amdgcn_readfirstlane ((int) (pos - base));
                  const uint32_t tq = (uint32_t) __builtin_amdgcn_readlane ((int) t, (int) at);
                  starts |= (uint64_t) 1 << at;
                  pos += (tq & MGD_MATCH) ? (tq >> 16) & 0x1ffu : 1u;
                }
              if ((starts >> lane) & 1)
                { const uint32_t idx = nTok + (uint32_t) __builtin_popcountll (starts & (((uint64_t) 1 << lane) - 1));
                  if (idx < n) tokens[idx] = t;
                  mgdCountToken (W, t);
                }
              nTok += (uint32_t) __builtin_popcountll (starts);
            }
        }
#else
      if (lane == 0)
        while (pos < s1 && nTok < n)
          { const uint32_t t = W->step[pos - s0];
            tokens[nTok++] = t;
            mgdCountToken (W, t);
            pos += (t & MGD_MATCH) ? (t >> 16) & 0x1ffu : 1u;
          }
#endif
      MGD_SYNC ();
    }
  if (lane == 0)
    { W->freqB[256] = 1; W->freqC[256] = 1;
      W->nTok = nTok;
    }
  MGD_SYNC ();

  /* ---- the costs: stored, literals only, with matches; the latter two with their own code and with the fixed one ---- */
  mgdMakeCode (W, &W->code[0], W->freqB, W->zero, 0, lane, nLanes);
  if (W->nMatch) mgdMakeCode (W, &W->code[1], W->freqC, W->distFreq, W->extraBits, lane, nLanes);
  if (lane == 0)
    { const uint32_t stored = 8 * (n + 5);
      uint32_t kind = 0, fixed = 0, bits = stored, fixB = 3, fixC = 3 + W->extraBits;
      for (i = 0 ; i < 286 ; ++i) { const uint32_t l = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8; fixB += W->freqB[i] * l; fixC += W->freqC[i] * l; }
      for (i = 0 ; i < 30 ; ++i) fixC += W->distFreq[i] * 5;
      if (W->code[0].bits < bits) { kind = 1; bits = W->code[0].bits; }
      if (fixB < bits) { kind = 1; fixed = 1; bits = fixB; }
      if (W->nMatch && W->code[1].bits < bits) { kind = 2; fixed = 0; bits = W->code[1].bits; }
      if (W->nMatch && fixC < bits) { kind = 2; fixed = 1; bits = fixC; }
      W->kind = kind; W->fixed = fixed; W->memberLen = 18 + (bits + 7) / 8 + 8;
      if (fixed)                                         /* the fixed code (RFC 1951 3.2.6) in the place of the one that lost to it */
        { MgDefCode *c = &W->code[kind - 1];
          const uint32_t *f = kind == 2 ? W->freqC : W->freqB;
          c->maxLit = 0; c->maxDist = kind == 2 ? 5 : 0; c->hdrBits = 3; c->bits = bits; c->nRle = 0;
          for (i = 0 ; i < 288 ; ++i)
            { c->litLen[i] = (uint8_t) (i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
              if (i < 286 && f[i] && c->litLen[i] > c->maxLit) c->maxLit = c->litLen[i];
            }
          for (i = 0 ; i < 32 ; ++i) c->distLen[i] = 5;
          mgdAssignCodes (W, c->litLen, 288, W->litCode); mgdAssignCodes (W, c->distLen, 32, W->distCode);
        }
      else if (kind)
        { const MgDefCode *c = &W->code[kind - 1];
          mgdAssignCodes (W, c->litLen, 286, W->litCode); mgdAssignCodes (W, c->distLen, 30, W->distCode); mgdAssignCodes (W, c->clLen, 19, W->clCode);
        }
      if (stats)
        { const MgDefCode *c = kind ? &W->code[kind - 1] : 0;
          stats[MGD_ST_KIND] = kind; stats[MGD_ST_LITERALS] = kind == 2 ? W->nTok - W->nMatch : n; stats[MGD_ST_MATCHES] = kind == 2 ? W->nMatch : 0;
          stats[MGD_ST_MATCH] = kind == 2 ? W->maxMatch : 0; stats[MGD_ST_DIST] = kind == 2 ? W->maxDist : 0;
          stats[MGD_ST_LITBITS] = c ? c->maxLit : 0; stats[MGD_ST_DISTBITS] = c ? c->maxDist : 0; stats[MGD_ST_BITS] = bits;
        }
    }
  MGD_SYNC ();

  /* ---- the member ---- */
  { const uint32_t kind = W->kind, memberLen = W->memberLen, words = (memberLen + 3) / 4;
    const uint64_t head0 = 0x0000000004088b1full, head1 = 0x000243420006ff00ull;      /* 1f 8b 08 04, mtime 0 | xfl 0, os ff, XLEN 6, 'B' 'C' 02 00 */
    for (i = lane ; i < words ; i += nLanes) mgdWordSet (out, i, 0);
    MGD_SYNC ();
    if (lane == 0) { mgdBytesOr (out, 0, head0, 8); mgdBytesOr (out, 8, head1, 8); mgdBytesOr (out, 16, memberLen - 1, 2); }
    if (!kind)
      { if (lane == 0) { mgdBytesOr (out, 18, 1, 1); mgdBytesOr (out, 19, n, 2); mgdBytesOr (out, 21, n ^ 0xffffu, 2); }
        MGD_SYNC ();                                     /* (the text's words are shared with nobody but its neighbours in this loop: all OR-ed) */
        for (i = lane ; i < n ; i += nLanes) mgdBytesOr (out, 23 + i, text[i], 1);
      }
    else
      { const MgDefCode *c = &W->code[kind - 1];
        const uint32_t items = (kind == 2 ? W->nTok : n) + 1, per = (items + nLanes - 1) / nLanes;
        const uint32_t a = lane * per < items ? lane * per : items, e = items - a < per ? items : a + per;
        uint32_t mine = 0, before = 0, k;
        MgdPut put;
        for (k = a ; k < e ; ++k) mine += mgdItemBits (c, k + 1 == items ? 256u : kind == 2 ? tokens[k] : text[k]);
        if (lane < MGD_MAX_LANES) W->laneBits[lane] = mine;
        if (lane == 0)                                   /* the block's header */
          { mgdPutStart (&put, out, 18 * 8);
            mgdPut (&put, 1, 1); mgdPut (&put, W->fixed ? 1 : 2, 2);
            if (!W->fixed) { mgdPut (&put, c->hlit - 257, 5); mgdPut (&put, c->hdist - 1, 5); mgdPut (&put, c->hclen - 4, 4); }
            for (k = 0 ; !W->fixed && k < c->hclen ; ++k) mgdPut (&put, c->clLen[mgdClOrder (k)], 3);
            for (k = 0 ; k < c->nRle ; ++k)
              { const uint32_t s = c->rle[k] & 0xffu, x = c->rle[k] >> 8;
                mgdPut (&put, W->clCode[s], c->clLen[s]);
                if (s == 16) mgdPut (&put, x, 2); else if (s == 17) mgdPut (&put, x, 3); else if (s == 18) mgdPut (&put, x, 7);
              }
            mgdPutEnd (&put);
          }
        MGD_SYNC ();
        for (k = 0 ; k < lane && k < MGD_MAX_LANES ; ++k) before += W->laneBits[k];
        if (a < e)
          { mgdPutStart (&put, out, 18 * 8 + c->hdrBits + before);
            for (k = a ; k < e ; ++k) mgdItemPut (&put, W, c, k + 1 == items ? 256u : kind == 2 ? tokens[k] : text[k]);
            mgdPutEnd (&put);
          }
      }
    /* ---- CRC-32 and length ---- */
    for (i = lane ; i < MGI_LANES ; i += nLanes) W->crcPart[i] = mgInfCrcSlice (W->crcTab, text, n, i);
    MGD_SYNC ();
    if (lane == 0)
      { uint32_t crc = 0;
        for (i = 0 ; i < MGI_LANES ; ++i) crc ^= W->crcPart[i];
        mgdBytesOr (out, memberLen - 8, crc, 4); mgdBytesOr (out, memberLen - 4, n, 4);
      }
    MGD_SYNC ();
    return memberLen;
  }
}

/* bgzip's end-of-file member: an empty member whose payload is the fixed-Huffman empty block */
#define MGD_EOF_BYTES 28
MGI_HD void mgDefEofMember (uint8_t *out28)
{
  const uint8_t e[MGD_EOF_BYTES] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
  uint32_t i;
  for (i = 0 ; i < MGD_EOF_BYTES ; ++i) out28[i] = e[i];
}
#endif
