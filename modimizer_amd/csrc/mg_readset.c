/* mg_readset.c — modasm's read ingest on top of the batch ABI:
 *   readsetFileRead (modasm.c:151-191)   scan + lookup of every read: one GPU batch call
 *   invBuild        (modasm.c:258-287)   per-mod lists of the reads that hit it
 *   readsetStats    (modasm.c:193-253)
 *   readsetWrite / readsetRead (modasm.c:108-149): <root>.mod + <root>.readset
 * The per-k-mer loop (modRCnext + modsetIndexFind) runs on the GPU (mgQueryReadsDevice); what is
 * left on the host is the reference's serial bookkeeping over the seeds — hit lists with the
 * orientation bit, 16-bit distances, saturating depth, copy-class tallies, the inverse lists —
 * restated with its quirks because the file and the printed statistics are the parity target.
 */
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "modgpu.h"
#include "mg_internal.h"

static double rsNowMs (void) { struct timespec t; clock_gettime (CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
#define RS_LAP(what) do { if (lapOn) { const double q_ = rsNowMs (); fprintf (stderr, "readset: %s %.2f ms\n", what, q_ - lap); lap = q_; } } while (0)      /* dev: MODGPU_SEED_TIMING=1 */

#define TOPBIT  0x80000000u        /* modasm.c:22: set for forward orientation */
#define TOPMASK 0x7fffffffu

static void fatal (const char *what)
{ fprintf (stderr, "FATAL ERROR: %s: %s\n", what, mgLastError ()); exit (-1); }

MgReadset *mgReadsetCreate (Modset *ms)                            /* modasm.c:90-98 */
{
  if (ms->max >= TOPBIT) { fprintf (stderr, "FATAL ERROR: too many entries in modset\n"); exit (-1); }   /* modasm.c:1562 */
  MgReadset *rs = (MgReadset *) calloc (1, sizeof (MgReadset));
  rs->ms = ms;
  rs->capReads = 1 << 16;
  rs->len = (int *) calloc ((size_t) rs->capReads, sizeof (int));
  rs->nHit = (int *) calloc ((size_t) rs->capReads, sizeof (int));
  rs->nMiss = (int *) calloc ((size_t) rs->capReads, sizeof (int));
  rs->nCopy = (int (*)[4]) calloc ((size_t) rs->capReads, sizeof (int[4]));
  rs->hitStart = (U64 *) calloc ((size_t) rs->capReads + 1, sizeof (U64));
  rs->bad = (U8 *) calloc ((size_t) rs->capReads, sizeof (U8));
  rs->contained = (int *) calloc ((size_t) rs->capReads, sizeof (int));
  return rs;
}

void mgReadsetDestroy (MgReadset *rs)
{
  if (!rs) return;
  free (rs->len); free (rs->nHit); free (rs->nMiss); free (rs->nCopy); free (rs->hitStart); free (rs->bad); free (rs->contained);
  mgReadsetDevForget (rs);
  free (rs->hit); free (rs->dx); free (rs->invStart); free (rs->invSpace); free (rs);
}

static void reserveReads (MgReadset *rs, int more)
{
  int need = rs->nReads + more + 2;
  if (need <= rs->capReads) return;
  int cap = rs->capReads; while (cap < need) cap *= 2;
  rs->len = (int *) realloc (rs->len, (size_t) cap * sizeof (int));
  rs->nHit = (int *) realloc (rs->nHit, (size_t) cap * sizeof (int));
  rs->nMiss = (int *) realloc (rs->nMiss, (size_t) cap * sizeof (int));
  rs->nCopy = (int (*)[4]) realloc (rs->nCopy, (size_t) cap * sizeof (int[4]));
  rs->hitStart = (U64 *) realloc (rs->hitStart, ((size_t) cap + 1) * sizeof (U64));
  rs->bad = (U8 *) realloc (rs->bad, (size_t) cap * sizeof (U8));
  rs->contained = (int *) realloc (rs->contained, (size_t) cap * sizeof (int));
  memset (rs->bad + rs->capReads, 0, (size_t) (cap - rs->capReads) * sizeof (U8));
  memset (rs->contained + rs->capReads, 0, (size_t) (cap - rs->capReads) * sizeof (int));
  rs->capReads = cap;
}

/* modasm.c:158: depth is rebuilt from the reads that follow.  The hits per mod are counted on the device across the batches of the
   file (mg_rsdev.hip); depth[] comes back, saturated, when the file is done */
static U32 *gDepthAccum (MgReadset *rs)
{
  U32 *d = 0;
  if (mgReadsetDevBegin (rs, rs->ms->max, &d)) fatal ("read set on the device");
  return d;
}
static U32 *readsetBegin (MgReadset *rs)
{
  if (modsetSyncToHost (rs->ms, 0)) fatal ("modsetSyncToHost");
  return gDepthAccum (rs);
}

/* modasm.c:161-188 for a batch of reads that is on the device (2-bit packed, offsets in bases) */
static void readsetAddBatchDevice (MgReadset *rs, U32 *dDepth, const void *dPacked, U64 total, const void *dOff, int nReads)
{
  Modset *ms = rs->ms;
  if (nReads <= 0) return;
  const int lapOn = mgKnobs ()->seedTiming == 1; double lap = lapOn ? rsNowMs () : 0;
  reserveReads (rs, nReads);
  int64_t *offsets = (int64_t *) malloc (((size_t) nReads + 1) * sizeof (int64_t));
  if (mgMemcpyD2H (offsets, dOff, ((size_t) nReads + 1) * 8, 0)) fatal ("D2H");
  /* scan, lookup, hit lists, distances and counts on the device (mg_chain.hip) */
  U64 *hStart = (U64 *) malloc (((size_t) nReads + 1) * sizeof (U64));
  U32 *hMiss = (U32 *) malloc (((size_t) nReads + 1) * sizeof (U32));
  U32 *dHit = 0; U16 *dDx = 0;
  if (mgReadsetSeedsDevice (ms, (const U32 *) dPacked, total, (const U64 *) dOff, (U32) nReads, hStart, hMiss, &dHit, &dDx, dDepth)) fatal ("read scan");
  const U64 n = hStart[nReads];
  RS_LAP ("batch: scan + lookups + hit lists");
  if (rs->totHit + n + 1 > rs->capHit)
    { rs->capHit = (rs->totHit + n + 1) * 2;
      rs->hit = (U32 *) realloc (rs->hit, rs->capHit * sizeof (U32));
      rs->dx = (U16 *) realloc (rs->dx, rs->capHit * sizeof (U16));
      if (!rs->hit || !rs->dx) { fprintf (stderr, "FATAL ERROR: out of memory\n"); exit (-1); }
      mgHugeHint (rs->hit, rs->capHit * sizeof (U32)); mgHugeHint (rs->dx, rs->capHit * sizeof (U16));      /* the lists arrive into fresh pages: one fault per 2 MiB, not per 4 KiB */
    }
  if (n && (mgCopyD2HBig (rs->hit + rs->totHit, dHit, (size_t) n * sizeof (U32)) || mgCopyD2HBig (rs->dx + rs->totHit, dDx, (size_t) n * sizeof (U16)))) fatal ("hit lists");
  RS_LAP ("batch: hit lists to the host");
  mgReadsetDevAppendHits (rs, dHit, n);              /* (the inverse lists are made from them on the device when the file is done) */
  mgDeviceFree (dHit); mgDeviceFree (dDx);
  const int first = rs->nReads + 1;                   /* reads are numbered from 1 (modasm.c:95) */
  for (int r = 0 ; r < nReads ; ++r)
    { const int id = first + r;
      rs->len[id] = (int) (offsets[r + 1] - offsets[r]);
      rs->nHit[id] = (int) (hStart[r + 1] - hStart[r]);
      rs->nMiss[id] = (int) hMiss[r];
      memset (rs->nCopy[id], 0, sizeof (int[4]));
      rs->bad[id] = 0; rs->contained[id] = 0;
      rs->hitStart[id] = rs->totHit + hStart[r];
    }
  rs->totHit += n;
  rs->nReads += nReads;
  rs->hitStart[rs->nReads + 1] = rs->totHit;
  free (hStart); free (hMiss); free (offsets);
  RS_LAP ("batch: per-read records");
}

/* ... from host bytes */
static void readsetAddBatch (MgReadset *rs, U32 *dDepth, const char *bases, const int64_t *offsets, int nReads)
{
  if (nReads <= 0) return;
  const int lapOn = mgKnobs ()->seedTiming == 1; double lap = lapOn ? rsNowMs () : 0;
  MgDevBatch b; mgBatchUpload (&b, bases, offsets, nReads);
  RS_LAP ("pack + upload");
  readsetAddBatchDevice (rs, dDepth, b.dPacked, b.total, b.dOff, nReads);
  mgBatchFree (&b);
  RS_LAP ("batch in all, + free");
}

/* invBuild (modasm.c:258-287) and the file's depth[] (modasm.c:174): on the device (mg_rsdev.hip: counts saturated, the lists a stable sort
   of the hits' read numbers by mod, a read's copy-class tallies a lane per read); a set of 2^32 hits or more takes the loops below */
static void readsetFinishHost (MgReadset *rs);
/* hitsBefore: rs->totHit when this file began.  A further file into a read set that holds hits already (modasm.c:158 zeroes depth[] per file
   and invBuild then walks ALL hits with the last file's depths: undefined in the reference): the device counted this file's hits alone, so
   depth[] and the lists are made from all the hits by the host loops, which agree with one another */
static void readsetFinish (MgReadset *rs, U64 hitsBefore)
{
  Modset *ms = rs->ms;
  free (rs->invStart); free (rs->invSpace); rs->invSpace = 0;
  rs->invStart = (U64 *) calloc ((size_t) ms->max + 2, sizeof (U64));
  mgHugeHint (rs->invStart, ((size_t) ms->max + 2) * sizeof (U64));
  if (rs->totHit >= 0xfffffff0ull || hitsBefore) { mgReadsetDevForget (rs); readsetFinishHost (rs); return; }
  if (mgReadsetFinishDevice (rs, ms, ms->max, rs->hit, rs->totHit, rs->hitStart, (U32) rs->nReads, ms->info, ms->depth, rs->invStart, &rs->invSpace, (int *) rs->nCopy))
    fatal ("read set on the device");                  /* (the device table's depth copy was set there too) */
}

/* the same by the reference's loops, for a set too large for 32-bit places (depth[] from the hits themselves) */
static void readsetFinishHost (MgReadset *rs)
{
  Modset *ms = rs->ms;
  memset (ms->depth, 0, ((size_t) ms->max + 1) * sizeof (U16));
  for (U64 h = 0 ; h < rs->totHit ; ++h)
    { U16 *dp = &ms->depth[rs->hit[h] & TOPMASK]; if (*dp < 0xffff) ++*dp; }      /* modasm.c:174 */
  mgModsetHostChanged (ms);
  rs->invSpace = (U32 *) malloc ((rs->totHit ? rs->totHit : 1) * sizeof (U32));
  U64 off = 0;
  for (U32 i = 1 ; i <= ms->max ; ++i)
    { rs->invStart[i] = off;
      if (ms->depth[i] && ms->depth[i] < 0xffff) off += ms->depth[i];
    }
  rs->invStart[ms->max + 1] = off;
  U64 *fill = (U64 *) malloc (((size_t) ms->max + 2) * sizeof (U64));
  memcpy (fill, rs->invStart, ((size_t) ms->max + 2) * sizeof (U64));
  for (int r = 1 ; r <= rs->nReads ; ++r)
    { int *nc = rs->nCopy[r];
      nc[0] = nc[1] = nc[2] = nc[3] = 0;               /* rebuilt here in case the copy classes changed */
      for (U64 h = rs->hitStart[r] ; h < rs->hitStart[r + 1] ; ++h)
        { const U32 y = rs->hit[h] & TOPMASK;
          ++nc[ms->info[y] & 3];
          if (ms->depth[y] < 0xffff) rs->invSpace[fill[y]++] = (U32) r;
        }
    }
  free (fill);
}

int mgReadsetRead (MgReadset *rs, const char *bases, const int64_t *offsets, int nReads)
{
  const int lapOn = mgKnobs ()->seedTiming == 1; double lap = lapOn ? rsNowMs () : 0;
  const U64 hitsBefore = rs->totHit;
  U32 *dDepth = readsetBegin (rs);
  RS_LAP ("begin");
  readsetAddBatch (rs, dDepth, bases, offsets, nReads);
  lap = lapOn ? rsNowMs () : 0;
  readsetFinish (rs, hitsBefore);
  RS_LAP ("finish");
  return 0;
}

typedef struct { MgReadset *rs; U32 *dDepth; } RsFileCtx;
static int rsDeviceBatch (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, void *stream)
{ RsFileCtx *c = (RsFileCtx *) v; (void) idBytes; (void) idOff; (void) stream; readsetAddBatchDevice (c->rs, c->dDepth, dPacked, total, dOff, (int) nReads); return 0; }
static int rsHostBatch (MgSeqBatch *b, void *v)
{ RsFileCtx *c = (RsFileCtx *) v; readsetAddBatch (c->rs, c->dDepth, b->bases, b->offsets, b->nSeq); return 0; }

int mgReadsetFileRead (MgReadset *rs, const char *filename)       /* modasm.c:151-191 */
{
  { FILE *f = fopen (filename, "rb"); if (!f) return -1; fclose (f); }
  const U64 hitsBefore = rs->totHit;
  RsFileCtx c; c.rs = rs; c.dDepth = readsetBegin (rs);
  /* plain FASTA / FASTQ text: parsed on the device (mg_textgpu.hip), the batches never exist as host bytes; gzip, a last line without
     its newline, FASTQ that breaks a rule: the host parser, from the first record the device parser has not handed on */
  const MgKnobs *kn = mgKnobs ();
  U64 nSeq = 0, totLen = 0, resumeOff = 0, resumeLine = 1;
  U64 batch = (U64) (kn->fileBatchMbp != MG_KNOB_UNSET && kn->fileBatchMbp > 0 ? kn->fileBatchMbp : 512) * 1000000;
  int rc = mgTextForEachBatchDevice (filename, rsDeviceBatch, &c, batch, 0, &nSeq, &totLen, &resumeOff, &resumeLine);
  if (rc == -2) rc = mgSeqForEachBatchFrom (filename, 0, 1, 0, rsHostBatch, &c);
  else if (rc == -3) rc = mgSeqForEachBatchFrom (filename, (size_t) resumeOff, resumeLine, nSeq, rsHostBatch, &c);
  /* a parser error after batches were appended: the reads that came are in rs (nReads, hit[] moved on), so depth[] / the inverse lists /
     nCopy[] are still made for them and the file's device buffers released -- rs is never left half built; the error goes back */
  readsetFinish (rs, hitsBefore);
  return rc;
}

void mgReadsetStats (MgReadset *rs, FILE *out)                     /* modasm.c:193-253 */
{
  Modset *ms = rs->ms;
  const U32 n = (U32) rs->nReads;
  if (!n) { fprintf (stderr, "stats called on empty readset\n"); return; }
  modsetSummary (ms, out);
  int nUnique0 = 0, nUnique1 = 0;
  U32 nBad[7] = { 0, 0, 0, 0, 0, 0, 0 };                            /* any, then one per flag of Read.bad (modasm.c:214-222) */
  U64 totLen = 0, totMiss = 0, lenUnique0 = 0, lenUnique1 = 0, totCopy[4] = { 0, 0, 0, 0 };
  for (U32 i = 1 ; i <= n ; ++i)
    { totLen += (U64) rs->len[i]; totMiss += (U64) rs->nMiss[i];
      for (int j = 0 ; j < 4 ; ++j) totCopy[j] += (U64) rs->nCopy[i][j];
      if (rs->nCopy[i][1] == 0) { ++nUnique0; lenUnique0 += (U64) rs->len[i]; }
      else if (rs->nCopy[i][1] == 1) { ++nUnique1; lenUnique1 += (U64) rs->len[i]; }
      if (rs->bad[i]) { ++nBad[0]; for (int j = 0 ; j < 6 ; ++j) if (rs->bad[i] & (1 << j)) ++nBad[1 + j]; }
    }
  fprintf (out, "RS %d sequences, total length %llu (av %.1f)\n", n, (unsigned long long) totLen, totLen / (double) n);
  fprintf (out, "RS %llu mod hits, %.1f bp/hit, frac hit %.2f, av hits/read %.1f\n",
           (unsigned long long) rs->totHit, totLen / (double) rs->totHit,
           rs->totHit / (double) (totMiss + rs->totHit), rs->totHit / (double) n);
  fprintf (out, "RS hit distribution %.2f copy0, %.2f copy1, %.2f copy2, %.2f copyM\n",
           totCopy[0] / (double) rs->totHit, totCopy[1] / (double) rs->totHit,
           totCopy[2] / (double) rs->totHit, totCopy[3] / (double) rs->totHit);
  const U32 nUniqueMulti = n - (U32) nUnique0 - (U32) nUnique1;
  fprintf (out, "RS num reads and av_len with 0 copy1 hits %d %.1f with 1 copy1 hits %d %.1f"
           " >1 copy1 hits %d %.1f av copy1 hits %.1f\n",
           nUnique0, lenUnique0 / (double) nUnique0, nUnique1, lenUnique1 / (double) nUnique1,
           nUniqueMulti, (totLen - lenUnique0 - lenUnique1) / (double) nUniqueMulti,
           (totCopy[1] - (U64) nUnique1) / (double) nUniqueMulti);
  fprintf (out, "RS bad %u : %u repeat, %u order10, %u order1, ", nBad[0], nBad[1], nBad[2], nBad[3]);      /* (set by the overlap passes below: zero after the ingest) */
  fprintf (out, "%u no_match, %u low_hit, %u low_copy1\n", nBad[4], nBad[5], nBad[6]);
  U32 nCopy[4] = { 0, 0, 0, 0 }, hitCopy[4] = { 0, 0, 0, 0 }, hit2Copy[4] = { 0, 0, 0, 0 };
  U64 depthCopy[4] = { 0, 0, 0, 0 };
  for (U32 i = 1 ; i <= ms->max ; ++i)
    { const int j = ms->info[i] & 3;
      ++nCopy[j];
      if (ms->depth[i] > 0) ++hitCopy[j];
      if (ms->depth[i] > 1) { ++hit2Copy[j]; depthCopy[j] += ms->depth[i]; }
    }
  static const char *label[4] = { "copy0", "copy1", "copy2", "copyM" };
  fprintf (out, "RS mod frac hit hit>1 av:");
  for (int j = 0 ; j < 4 ; ++j)
    fprintf (out, " %s %.3f %.3f %.1f", label[j], hitCopy[j] / (double) nCopy[j], hit2Copy[j] / (double) nCopy[j],
             depthCopy[j] / (double) hit2Copy[j]);
  fprintf (out, "\n");
}

/* ---- <root>.mod + <root>.readset (modasm.c:108-149) ---- */

/* one element of the reference's Array of Read (modasm.c:30-57), 72 bytes; hit and dx are the
 * addresses of the read's lists in the writing process, meaningless in a file */
typedef struct {
  int len, nHit; U64 hitPtr, dxPtr; U8 bad, otherFlags; U16 pad1; int nMiss, contained, nCopy[4]; U32 pad2[4]; U32 tail;
} FileRead;
typedef struct { int magic, pad0; U64 base; int dim, size, max, pad1; } FileArray;   /* array.h:41-50 */
#define FILE_ARRAY_MAGIC 8918274

static void die1 (const char *fmt, const char *arg)
{ fprintf (stderr, "FATAL ERROR: "); fprintf (stderr, fmt, arg); fprintf (stderr, "\n"); exit (-1); }
#define WR(ptr, sz, cnt, what) do { if (fwrite ((ptr), (sz), (cnt), f) != (size_t) (cnt)) die1 ("failed to write %s", what); } while (0)
#define RD(ptr, sz, cnt, what) do { if (fread ((ptr), (sz), (cnt), f) != (size_t) (cnt)) die1 ("failed to read %s", what); } while (0)

/* invBuild (modasm.c:258-287) by its loops from ms->depth and ms->info as they are, for hit lists that came from a file or whose modset the
   caller has worked on: a hit beyond the modset is fatal (root: the file it came from, or 0), and a list never runs past the hits there are */
static void readsetInvBuildHost (MgReadset *rs, const char *root)
{
  Modset *m = rs->ms;
  free (rs->invStart); free (rs->invSpace);
  rs->invStart = (U64 *) calloc ((size_t) m->max + 2, sizeof (U64));
  rs->invSpace = (U32 *) malloc ((rs->totHit ? rs->totHit : 1) * sizeof (U32));
  U64 off = 0;
  for (U32 i = 1 ; i <= m->max ; ++i) { rs->invStart[i] = off; if (m->depth[i] && m->depth[i] < 0xffff) off += m->depth[i]; }
  rs->invStart[m->max + 1] = off;
  U64 *fill = (U64 *) malloc (((size_t) m->max + 2) * sizeof (U64));
  memcpy (fill, rs->invStart, ((size_t) m->max + 2) * sizeof (U64));
  for (int r = 1 ; r <= rs->nReads ; ++r)
    { int *nc = rs->nCopy[r]; nc[0] = nc[1] = nc[2] = nc[3] = 0;
      for (U64 h = rs->hitStart[r] ; h < rs->hitStart[r + 1] ; ++h)
        { const U32 y = rs->hit[h] & TOPMASK;
          if (y > m->max) { if (root) die1 ("hit beyond the modset in %s.readset", root); die1 ("hit beyond the modset in %s", "the read set"); }
          ++nc[m->info[y] & 3];
          if (m->depth[y] < 0xffff && fill[y] < rs->totHit) rs->invSpace[fill[y]++] = (U32) r;
        }
    }
  free (fill);
}

void mgReadsetWrite (MgReadset *rs, const char *root)              /* modasm.c:108-126 */
{
  FILE *f;
  if (!(f = mgTagOpen (root, "mod", "w"))) die1 ("can't open file %s.mod", root);
  modsetWrite (rs->ms, f); fclose (f);
  if (!(f = mgTagOpen (root, "readset", "w"))) die1 ("can't open file %s.readset", root);
  WR ("RSMSHv2", 8, 1, "readset header");
  WR (&rs->totHit, sizeof (U64), 1, "totHit");
  FileArray ah; memset (&ah, 0, sizeof (ah));
  ah.magic = FILE_ARRAY_MAGIC; ah.size = (int) sizeof (FileRead); ah.max = rs->nReads + 1;
  ah.dim = mgRefArrayDim (1 << 16, (int) sizeof (FileRead), rs->nReads + 1);           /* readsetCreate (ms, 1<<16), modasm.c:1568 */
  WR (&ah, sizeof (ah), 1, "reads");
  FileRead *recs = (FileRead *) calloc ((size_t) ah.dim, sizeof (FileRead));
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { recs[i].len = rs->len[i]; recs[i].nHit = rs->nHit[i]; recs[i].nMiss = rs->nMiss[i];
      recs[i].bad = rs->bad[i]; recs[i].contained = rs->contained[i];
      memcpy (recs[i].nCopy, rs->nCopy[i], sizeof (int[4]));
    }
  WR (recs, sizeof (FileRead), ah.dim, "reads");
  free (recs);
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { const U64 a = rs->hitStart[i], n = rs->hitStart[i + 1] - a;
      if (!n) continue;
      WR (rs->hit + a, sizeof (U32), n, "hits");
      WR (rs->dx + a, sizeof (U16), n, "dx");
    }
  if (fclose (f)) die1 ("failed to close %s.readset", root);
}

MgReadset *mgReadsetLoad (const char *root)                        /* modasm.c:128-149 */
{
  FILE *f;
  if (!(f = mgTagOpen (root, "mod", "r"))) die1 ("can't open file %s.mod", root);
  Modset *ms = modsetRead (f); fclose (f);
  if (!(f = mgTagOpen (root, "readset", "r"))) die1 ("can't open file %s.readset", root);
  char tag[8]; RD (tag, 8, 1, "readset header");
  if (memcmp (tag, "RSMSHv2", 8)) die1 ("bad readset header %s != RSMSHv2", tag);
  MgReadset *rs = mgReadsetCreate (ms);
  RD (&rs->totHit, sizeof (U64), 1, "totHit");
  FileArray ah; RD (&ah, sizeof (ah), 1, "reads");
  if (ah.magic != FILE_ARRAY_MAGIC || ah.size != (int) sizeof (FileRead) || ah.max < 1 || ah.dim < ah.max) die1 ("bad reads array in %s.readset", root);
  FileRead *recs = (FileRead *) malloc ((size_t) ah.dim * sizeof (FileRead));
  RD (recs, sizeof (FileRead), ah.dim, "reads");
  reserveReads (rs, ah.max);
  rs->nReads = ah.max - 1;
  rs->capHit = rs->totHit + 1;
  rs->hit = (U32 *) malloc (rs->capHit * sizeof (U32));
  rs->dx = (U16 *) malloc (rs->capHit * sizeof (U16));
  U64 at = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { rs->len[i] = recs[i].len; rs->nHit[i] = recs[i].nHit; rs->nMiss[i] = recs[i].nMiss;
      rs->bad[i] = recs[i].bad; rs->contained[i] = recs[i].contained;
      memcpy (rs->nCopy[i], recs[i].nCopy, sizeof (int[4]));
      rs->hitStart[i] = at;
      const U64 n = (U64) recs[i].nHit;
      if (recs[i].nHit < 0 || at + n > rs->totHit) die1 ("bad hit counts in %s.readset", root);
      if (n) { RD (rs->hit + at, sizeof (U32), n, "hits"); RD (rs->dx + at, sizeof (U16), n, "dx"); }
      at += n;
    }
  rs->hitStart[rs->nReads + 1] = at;
  free (recs);
  fclose (f);
  readsetInvBuildHost (rs, root);                    /* invBuild as readsetRead does (modasm.c:147), from the depth the .mod file carries */
  return rs;
}

/* ---- modasm -C and -P (cleanMods, modasm.c:514-555; readProperties, modasm.c:912-952) ----
 * Both ask how often one read holds one mod; the reference clears an array of ms->max + 1 entries per read to find out.  On the device
 * (mg_rsdev.hip) the hits are sorted by mod; the host loops below, for a set of 2^32 - 16 hits or more, a device without room or
 * MODGPU_READSET_HOST=1, stamp the array with the read's number instead of clearing it.  Same bytes either way. */

static __thread int gCleanPath = -1, gPropertiesPath = -1;
int mgReadsetCleanModsPath (void) { return gCleanPath; }
int mgReadsetPropertiesPath (void) { return gPropertiesPath; }
static int rsHostForced (const MgReadset *rs) { return rs->totHit >= 0xfffffff0ull || mgKnobs ()->readsetHost == 1; }

static void cleanModsHost (MgReadset *rs, U32 counts[3])
{
  Modset *ms = rs->ms;
  const int w = ms->hasher->w;
  U32 *inRead = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32));      /* the last read (from 1) that held the mod */
  for (int r = 1 ; r < rs->nReads ; ++r)                                   /* modasm.c:522-523: the last read is never looked at */
    { const U64 a = rs->hitStart[r], e = rs->hitStart[r + 1];
      for (U64 h = a ; h < e ; ++h)
        { const U32 hh = rs->hit[h] & TOPMASK;
          if (inRead[hh] == (U32) r) msSetRepeat (ms, hh);
          inRead[hh] = (U32) r;
          if (h == a) continue;
          if ((int) rs->dx[h] < w && h + 1 < e && (int) rs->dx[h + 1] < w) msSetInternal (ms, hh);
          const U32 hhLast = rs->hit[h - 1] & TOPMASK;
          const int lastDepth = ms->depth[hhLast], thisDepth = ms->depth[hh];
          if (lastDepth > 2 * thisDepth) msSetMinor (ms, hh);
          if (thisDepth > 2 * lastDepth) msSetMinor (ms, hhLast);
        }
    }
  free (inRead);
  counts[0] = counts[1] = counts[2] = 0;
  for (U64 i = 0 ; i <= ms->max ; ++i)
    { if (msIsRepeat (ms, i)) ++counts[0];
      if (msIsInternal (ms, i)) ++counts[1];
      if (msIsMinor (ms, i)) ++counts[2];
    }
  for (int r = 1 ; r <= rs->nReads ; ++r)                                  /* invBuild's nCopy[] (modasm.c:273-277) */
    { int *nc = rs->nCopy[r]; nc[0] = nc[1] = nc[2] = nc[3] = 0;
      for (U64 h = rs->hitStart[r] ; h < rs->hitStart[r + 1] ; ++h) ++nc[ms->info[rs->hit[h] & TOPMASK] & 3];
    }
}

int mgReadsetCleanMods (MgReadset *rs, FILE *out)                 /* modasm.c:514-555 */
{
  gCleanPath = -1;
  Modset *ms = rs->ms;
  if (modsetSyncToHost (ms, 0)) return -1;
  U32 counts[3] = { 0, 0, 0 };
  int host = rsHostForced (rs);
  if (!host)
    { const int rc = mgReadsetCleanDevice (ms->max, ms->hasher->w, rs->hit, rs->dx, rs->totHit, rs->hitStart, (U32) rs->nReads, ms->depth, ms->info, (int *) rs->nCopy, counts);
      if (rc < 0) return -1;
      host = rc;
    }
  if (host) cleanModsHost (rs, counts);
  gCleanPath = host;
  /* invBuild (modasm.c:552): the lists are a function of the hits and of depth[]; they are made again only if depth[] no longer gives the places held */
  { U64 off = 0; int same = rs->invStart && rs->invSpace;
    for (U32 i = 1 ; same && i <= ms->max ; ++i) { same = rs->invStart[i] == off; if (ms->depth[i] && ms->depth[i] < 0xffff) off += ms->depth[i]; }
    if (!same || rs->invStart[ms->max + 1] != off) readsetInvBuildHost (rs, 0);
  }
  mgModsetHostChanged (ms);                                        /* info[] is new: a device table is made again from the host arrays on its next use */
  fprintf (out, "set %d repeated, %d internal, %d minor_variant mods\n", (int) counts[0], (int) counts[1], (int) counts[2]);
  return 0;
}

typedef struct { U32 *ev; U32 n, cap; } RsEvents;      /* triples (read, mod | TOPBIT if in one orientation, count) */
static int rsU32Cmp (const void *a, const void *b) { const U32 x = *(const U32 *) a, y = *(const U32 *) b; return x < y ? -1 : x > y; }

static void propertiesHost (MgReadset *rs, int *tally, RsEvents *E)
{
  Modset *ms = rs->ms;
  U32 *f = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32)), *r = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32));
  U32 *seen = 0; U64 capSeen = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { const U64 a = rs->hitStart[i], e = rs->hitStart[i + 1];
      if (e - a > capSeen) { capSeen = e - a; seen = (U32 *) realloc (seen, capSeen * sizeof (U32)); }
      U64 nSeen = 0;
      for (U64 j = a ; j < e ; ++j)
        { const U32 h = rs->hit[j] & TOPMASK;
          if (!msIsCopy1 (ms, h)) continue;
          if (!f[h] && !r[h]) seen[nSeen++] = h;
          if (rs->hit[j] & TOPBIT) ++f[h]; else ++r[h];
        }
      qsort (seen, nSeen, sizeof (U32), rsU32Cmp);                  /* distinct mods: any sort gives the one ascending order */
      int *t = tally + 5 * (size_t) i;
      for (U64 q = 0 ; q < nSeen ; ++q)
        { const U32 h = seen[q], nf = f[h], nr = r[h];
          f[h] = r[h] = 0;
          ++t[0];
          if (nf + nr == 1) continue;
          if (nf == 1 && nr == 1) ++t[2];
          else if (nf + nr == 2) ++t[1];
          else
            { const int tan = !nf || !nr;
              ++t[tan ? 3 : 4];
              if (E->n == E->cap) { E->cap = E->cap ? E->cap * 2 : 1024; E->ev = (U32 *) realloc (E->ev, (size_t) E->cap * 12); }
              U32 *v = E->ev + 3 * (size_t) E->n++;
              v[0] = (U32) i; v[1] = h | (tan ? TOPBIT : 0); v[2] = nf + nr;
            }
        }
    }
  free (f); free (r); free (seen);
}

int mgReadsetProperties (MgReadset *rs, FILE *out)                /* modasm.c:912-952 */
{
  gPropertiesPath = -1;
  Modset *ms = rs->ms;
  if (modsetSyncToHost (ms, 0)) return -1;
  int *tally = (int *) calloc (((size_t) rs->nReads + 1) * 5, sizeof (int));      /* per read { n, n2Tan, n2Rev, nMoreTan, nMoreRev } */
  RsEvents E = { 0, 0, 0 };
  int host = rsHostForced (rs);
  if (!host)
    { const int rc = mgReadsetPropertiesDevice (ms->max, rs->hit, rs->totHit, rs->hitStart, (U32) rs->nReads, ms->info, tally, &E.ev, &E.n);
      if (rc < 0) { free (tally); return -1; }
      host = rc;
    }
  if (host) propertiesHost (rs, tally, &E);
  gPropertiesPath = host;
  /* the lines (one short one per read, and one per mod that a read holds more than twice in one orientation): the events are in (read, mod) order */
  U32 e = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { const int *t = tally + 5 * (size_t) i;
      const U32 e0 = e;
      for ( ; e < E.n && E.ev[3 * (size_t) e] == (U32) i ; ++e)
        if (E.ev[3 * (size_t) e + 1] & TOPBIT) fprintf (out, "MT i %d h %d count %d\n", i, (int) (E.ev[3 * (size_t) e + 1] & TOPMASK), (int) E.ev[3 * (size_t) e + 2]);
      fprintf (out, "READ %d n %d n2Tan %d n2Rev %d nMoreTan %d nMoreRev %d\n", i, t[0], t[1], t[2], t[3], t[4]);
      if (t[3] > 5)
        { fprintf (out, "RM %d nMoreTan %d", i, t[3]);
          for (U32 j = e0 ; j < e ; ++j) fprintf (out, " %d", (int) (E.ev[3 * (size_t) j + 1] & TOPMASK));
          fputc ('\n', out);
        }
    }
  free (tally); free (E.ev);
  return 0;
}

/* ---- modasm -o1 / -o2 / -b / -c: findOverlaps (modasm.c:314-418) and its callers markBadReads (1266-1322), markContained (1370-1394) ----
 * findOverlaps (x) splits into a record per partner y that depends on the two hit lists and on info[] / depth[] alone -- made for a batch of queries
 * at once, on the device (mg_overlap.hip) or by the loops below -- and a replay that reads and writes the reads' `bad` in the order of the calls
 * (ovlReplay).  The host loops stamp their per-mod and per-read arrays with the query's serial number where the reference clears them per call. */

static __thread int gOverlapsPath = -1;
static __thread U64 gOverlapsDiag[4];
int mgReadsetOverlapsPath (void) { return gOverlapsPath; }
void mgReadsetOverlapsDiag (U64 out4[4]) { memcpy (out4, gOverlapsDiag, sizeof (gOverlapsDiag)); }

enum { BAD_REPEAT = 1, BAD_ORDER10 = 2, BAD_ORDER1 = 4, BAD_NOMATCH = 8, BAD_LOWHIT = 16, BAD_LOWCOPY1 = 32 };      /* modasm.c:38-45 */
enum { OVL_PLUS = 1, OVL_CONTAINED = 2, OVL_SKIPPED = 4 };

typedef struct { U32 iy, nHit; U64 first; } OvlCand;
typedef struct {
  U32 *modStamp, *readStamp, *readSlot; U16 *modJ;      /* hmap / omap of modasm.c:317-321, valid where the stamp is the query's */
  U32 stamp;
  OvlCand *cand; U64 capCand;
  int64_t *xPos; U64 capPos;
} OvlHost;

static int ovlCandCmp (const void *a, const void *b)     /* nHit descending, equal nHit in arrival order: what the reference's sort by nHit alone leaves (glibc's qsort is a stable merge sort) */
{
  const OvlCand *x = (const OvlCand *) a, *y = (const OvlCand *) b;
  if (x->nHit != y->nHit) return x->nHit > y->nHit ? -1 : 1;
  return x->first < y->first ? -1 : x->first > y->first;
}

/* the record of (x, y): modasm.c:359-390 in one walk of y's hits.  Both order tests are counted (they depend on the sequence of matches alone), the
   majority picks one afterwards */
static void ovlPairHost (const MgReadset *rs, const OvlHost *H, U32 x, U32 y, MgOvlRec *r)
{
  const U64 ax = rs->hitStart[x], ay = rs->hitStart[y], ey = rs->hitStart[y + 1];
  U32 nPlus = 0, nMinus = 0, nLess = 0, nGreater = 0, lastLess = 0, lastGreater = (U32) rs->nHit[x];
  int64_t yPos = 0, firstDiff = 0, lastDiff = 0; int any = 0;
  for (U64 h = ay ; h < ey ; ++h)
    { const U32 hy = rs->hit[h], m = hy & TOPMASK;
      yPos += rs->dx[h];
      if (H->modStamp[m] != H->stamp) continue;
      const U32 ihx = H->modJ[m];                                    /* j + 1 */
      if ((hy & TOPBIT) == (rs->hit[ax + ihx - 1] & TOPBIT)) ++nPlus; else ++nMinus;
      lastDiff = H->xPos[ihx] - yPos;
      if (!any) { firstDiff = lastDiff; any = 1; }
      if (ihx < lastLess) ++nLess;
      if (ihx > lastGreater) ++nGreater;
      lastLess = lastGreater = ihx;
    }
  r->nBadOrder = r->nBadFlip = r->flags = 0;
  if (nPlus > nMinus)
    { r->flags = OVL_PLUS; r->nBadFlip = (U16) nMinus; r->nBadOrder = (U16) nLess; nPlus -= nLess;
      if (firstDiff < 0 && !((int64_t) rs->len[x] - lastDiff > (int64_t) rs->len[y])) r->flags |= OVL_CONTAINED;
    }
  else if (nMinus && !nPlus) { r->nBadOrder = (U16) nGreater; nMinus -= nGreater; }      /* (isContained cannot be set here: modasm.c:382,386) */
  r->nPlus = (U16) nPlus; r->nMinus = (U16) nMinus;
}

typedef struct { MgOvlRec *recs; U64 n, cap; } OvlRecs;
static MgOvlRec *ovlRecsRoom (OvlRecs *R, U64 more)
{
  if (R->n + more > R->cap) { R->cap = (R->n + more) * 2 + 64; R->recs = (MgOvlRec *) realloc (R->recs, R->cap * sizeof (MgOvlRec)); }
  return R->recs ? R->recs + R->n : 0;
}

static int ovlBatchHost (const MgReadset *rs, OvlHost *H, const U32 *queries, U32 nq, U32 *nRepeat, U64 *start, MgOvlRec **recsOut, U64 diag[4])
{
  const Modset *ms = rs->ms;
  OvlRecs R = { 0, 0, 0 };
  for (U32 q = 0 ; q < nq ; ++q)
    { const U32 x = queries[q];
      const U64 ax = rs->hitStart[x], nx = rs->hitStart[x + 1] - ax;
      ++H->stamp;
      if (nx + 1 > H->capPos) { H->capPos = nx + 1; H->xPos = (int64_t *) realloc (H->xPos, H->capPos * sizeof (int64_t)); if (!H->xPos) return -1; }
      U64 nCand = 0, walked = 0; U32 rep = 0;
      H->xPos[0] = 0;
      for (U64 j = 0 ; j < nx ; ++j)
        { const U32 m = rs->hit[ax + j] & TOPMASK;
          H->xPos[j + 1] = H->xPos[j] + rs->dx[ax + j];
          if ((ms->info[m] & 3) != 1) continue;
          if (H->modStamp[m] == H->stamp) { ++rep; continue; }
          H->modStamp[m] = H->stamp; H->modJ[m] = (U16) (j + 1);
          for (U64 k = rs->invStart[m] ; k < rs->invStart[m + 1] ; ++k, ++walked)
            { const U32 y = rs->invSpace[k];
              if (H->readStamp[y] != H->stamp)
                { H->readStamp[y] = H->stamp; H->readSlot[y] = (U32) nCand;
                  if (nCand == H->capCand) { H->capCand = H->capCand ? H->capCand * 2 : 256; H->cand = (OvlCand *) realloc (H->cand, H->capCand * sizeof (OvlCand)); if (!H->cand) return -1; }
                  H->cand[nCand].iy = y; H->cand[nCand].nHit = 0; H->cand[nCand].first = walked; ++nCand;
                }
              ++H->cand[H->readSlot[y]].nHit;
            }
        }
      nRepeat[q] = rep; start[q] = R.n; diag[1] += walked;
      qsort (H->cand, nCand, sizeof (OvlCand), ovlCandCmp);
      U64 keep = 0; while (keep < nCand && H->cand[keep].nHit >= 3) ++keep;
      MgOvlRec *r = ovlRecsRoom (&R, keep + 1);
      if (!r) return -1;
      for (U64 c = 0 ; c < keep ; ++c) { r[c].iy = H->cand[c].iy; r[c].nHit = (U16) H->cand[c].nHit; ovlPairHost (rs, H, x, r[c].iy, &r[c]); }
      R.n += keep; diag[2] += keep;
    }
  start[nq] = R.n;
  if (!R.recs) R.recs = (MgOvlRec *) malloc (sizeof (MgOvlRec));
  *recsOut = R.recs;
  return 0;
}

/* findOverlaps (x, level) from x's records: what depends on the flags as they are now (modasm.c:336,358,391-415).  A skipped record is left as -b / -c
   see it: zero counts and flags */
static void ovlReplay (MgReadset *rs, U32 x, U32 nRepeat, MgOvlRec *recs, U64 n, int level, FILE *out)
{
  if (nRepeat) rs->bad[x] |= BAD_REPEAT;
  int nGood = 0, nBad = 0;
  for (U64 i = 0 ; i < n ; ++i)
    { MgOvlRec *o = &recs[i];
      if (rs->bad[o->iy]) { o->nBadOrder = o->nBadFlip = 0; o->flags = OVL_SKIPPED; continue; }
      const int isBad = o->nBadOrder || o->nBadFlip;
      if (isBad) ++nBad; else ++nGood;
      if (level > 1 && out)
        fprintf (out, "RH\t%u\tlen %d\t%s\t+ %d\t- %d\tbadOrder %d\t%s\n", o->iy, rs->len[o->iy], isBad ? "BAD" : "GOOD", (int) o->nPlus, (int) o->nMinus, (int) o->nBadOrder,
                 (o->flags & OVL_CONTAINED) ? "CONTAINED" : "OVERLAP");
    }
  if (!nGood && !nBad)
    { rs->bad[x] |= BAD_NOMATCH;
      if (rs->nHit[x] < 10) rs->bad[x] |= BAD_LOWHIT;
      else if (rs->nCopy[x][1] < 10) rs->bad[x] |= BAD_LOWCOPY1;
    }
  if (level > 0 && out)
    { fprintf (out, "RR %6u\tlen %d\tnHit %3d\tnMiss %3d\t", x, rs->len[x], rs->nHit[x], rs->nMiss[x]);
      fprintf (out, "nCpy %d %d %d %d\t", rs->nCopy[x][0], rs->nCopy[x][1], rs->nCopy[x][2], rs->nCopy[x][3]);
      fprintf (out, "nRepeatMod %d\tnGood %4d\tnBad %4d\n", (int) nRepeat, nGood, nBad);
    }
}

void mgOverlapsFree (MgOverlaps *res)
{
  if (!res) return;
  free (res->start); free (res->iy); free (res->nHit); free (res->nBadOrder); free (res->nBadFlip); free (res->flags);
  memset (res, 0, sizeof (*res));
}

typedef void (*OvlEach) (void *ctx, U32 x, const MgOvlRec *recs, U64 n);

/* the queries in the order given: checks, batches by the candidate budget, per batch the records (device or host loops), then the replay of its queries
   in order before the next batch's records are made -- the records do not read the flags, so only the replay is ordered */
static int ovlDrive (MgReadset *rs, const U32 *reads, U32 n, int level, FILE *out, MgOverlaps *res, OvlEach each, void *ctx)
{
  Modset *ms = rs->ms;
  const U32 nReads = (U32) rs->nReads;
  if (res) memset (res, 0, sizeof (*res));
  if (modsetSyncToHost (ms, 0)) return -1;
  if (!rs->invStart || !rs->invSpace) { mgSetErrorText ("overlaps: the read set has no inverse lists (nothing was read into it)"); return -1; }
  for (U32 i = 1 ; i <= nReads ; ++i)
    if (rs->nHit[i] > 65534 || rs->hitStart[i + 1] - rs->hitStart[i] > 65534)
      { char msg[160]; snprintf (msg, sizeof (msg), "overlaps: read %u has more than 65534 hits (the reference's 16-bit hit numbers wrap there)", i); mgSetErrorText (msg); return -1; }
  U64 *bound = (U64 *) malloc (((size_t) n + 1) * sizeof (U64));      /* per query: its candidates, repeats' lists counted too */
  U64 maxBound = 0;
  for (U32 q = 0 ; q < n ; ++q)
    { const U32 x = reads[q];
      if (x < 1 || x > nReads)
        { char msg[160]; snprintf (msg, sizeof (msg), "overlaps: read %u is not in the read set (reads 1 .. %u)", x, nReads); mgSetErrorText (msg); free (bound); return -1; }
      U64 b = 0;
      for (U64 h = rs->hitStart[x] ; h < rs->hitStart[x + 1] ; ++h)
        { const U32 m = rs->hit[h] & TOPMASK;
          if ((ms->info[m] & 3) != 1) continue;
          if (ms->depth[m] == 0xffff)
            { char msg[200]; snprintf (msg, sizeof (msg), "overlaps: copy-1 mod %u of read %u has a saturated depth and so no inverse list (modasm.c:266,338)", m, x); mgSetErrorText (msg); free (bound); return -1; }
          b += rs->invStart[m + 1] - rs->invStart[m];
        }
      bound[q] = b; if (b > maxBound) maxBound = b;
    }
  const MgKnobs *kn = mgKnobs ();
  int host = rsHostForced (rs) || maxBound >= 0x7fffffffull;
  MgOvlDev *dev = 0;
  if (!host)
    { const int rc = mgOvlDevOpen (&dev, ms->max, ms->info, rs->hit, rs->dx, rs->totHit, rs->hitStart, rs->len, nReads, rs->invStart, rs->invSpace);
      if (rc < 0) { free (bound); return -1; }
      host = rc;
    }
  U64 budget = kn->overlapCands != MG_KNOB_UNSET && kn->overlapCands > 0 ? (U64) kn->overlapCands : host ? (U64) 1 << 24 : mgOvlDevCandBudget ();
  if (budget > 0x7fffffffull) budget = 0x7fffffffull;
  OvlHost H; memset (&H, 0, sizeof (H));
  MgOverlaps R; memset (&R, 0, sizeof (R));
  U64 capRes = 0, nRes = 0;
  int rc = 0;
  if (res) { R.n = n; R.start = (U64 *) calloc ((size_t) n + 1, sizeof (U64)); }
  U32 *nRepeat = 0; U64 *start = 0; U32 capQ = 0;
  for (U32 q0 = 0 ; q0 < n && !rc ; )
    { U32 q1 = q0; U64 cands = 0, hits = 0;
      while (q1 < n && (q1 == q0 || (cands + bound[q1] <= budget && hits + (U64) rs->nHit[reads[q1]] < 0x7fffffffull && q1 - q0 < (1u << 24))))
        { cands += bound[q1]; hits += (U64) rs->nHit[reads[q1]]; ++q1; }
      const U32 nq = q1 - q0;
      if (nq > capQ) { capQ = nq; nRepeat = (U32 *) realloc (nRepeat, (size_t) capQ * sizeof (U32)); start = (U64 *) realloc (start, ((size_t) capQ + 1) * sizeof (U64)); }
      MgOvlRec *recs = 0;
      if (!host)
        { const int d = mgOvlDevBatch (dev, reads + q0, nq, nRepeat, start, &recs, gOverlapsDiag);
          if (d < 0) { rc = -1; break; }
          if (d > 0) { host = 1; mgOvlDevClose (dev); dev = 0; }      /* no room for this batch: the host loops, from here on */
        }
      if (host)
        { if (!H.modStamp)
            { H.modStamp = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32)); H.modJ = (U16 *) calloc ((size_t) ms->max + 1, sizeof (U16));
              H.readStamp = (U32 *) calloc ((size_t) nReads + 1, sizeof (U32)); H.readSlot = (U32 *) calloc ((size_t) nReads + 1, sizeof (U32));
              if (!H.modStamp || !H.modJ || !H.readStamp || !H.readSlot) { mgSetErrorText ("overlaps: out of memory"); rc = -1; break; }
            }
          if (ovlBatchHost (rs, &H, reads + q0, nq, nRepeat, start, &recs, gOverlapsDiag)) { mgSetErrorText ("overlaps: out of memory"); rc = -1; break; }
        }
      ++gOverlapsDiag[0];
      for (U32 q = 0 ; q < nq ; ++q)
        { const U32 x = reads[q0 + q];
          MgOvlRec *r = recs + start[q]; const U64 nr = start[q + 1] - start[q];
          ovlReplay (rs, x, nRepeat[q], r, nr, level, out);
          if (each) each (ctx, x, r, nr);
          if (res)
            { if (nRes + nr > capRes)
                { capRes = (nRes + nr) * 2 + 64;
                  R.iy = (U32 *) realloc (R.iy, capRes * sizeof (U32)); R.nHit = (U16 *) realloc (R.nHit, capRes * sizeof (U16)); R.nBadOrder = (U16 *) realloc (R.nBadOrder, capRes * sizeof (U16));
                  R.nBadFlip = (U16 *) realloc (R.nBadFlip, capRes * sizeof (U16)); R.flags = (U8 *) realloc (R.flags, capRes * sizeof (U8));
                }
              for (U64 i = 0 ; i < nr ; ++i)
                { R.iy[nRes + i] = r[i].iy; R.nHit[nRes + i] = r[i].nHit; R.nBadOrder[nRes + i] = r[i].nBadOrder; R.nBadFlip[nRes + i] = r[i].nBadFlip; R.flags[nRes + i] = (U8) r[i].flags; }
              nRes += nr; R.start[q0 + q + 1] = nRes;
            }
        }
      free (recs);
      q0 = q1;
    }
  if (dev) mgOvlDevClose (dev);
  free (H.modStamp); free (H.modJ); free (H.readStamp); free (H.readSlot); free (H.cand); free (H.xPos);
  free (nRepeat); free (start); free (bound);
  if (rc) { mgOverlapsFree (&R); return -1; }
  if (res) *res = R;
  gOverlapsPath = host;
  return 0;
}

int mgReadsetFindOverlaps (MgReadset *rs, const U32 *reads, U32 n, int level, FILE *out, MgOverlaps *res)
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  return ovlDrive (rs, reads, n, level, out, res, 0, 0);
}

int mgReadsetOverlapStats (MgReadset *rs, U32 d, FILE *out)         /* modasm.c:1586-1592 */
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  if (!d) { mgSetErrorText ("overlaps: -o2 0 never ends in the reference; the step is at least 1"); return -1; }
  const U32 n = (U32) rs->nReads / d;
  U32 *reads = (U32 *) malloc (((size_t) n + 1) * sizeof (U32));
  for (U32 i = 0 ; i < n ; ++i) reads[i] = (i + 1) * d;
  const int rc = ovlDrive (rs, reads, n, 1, out, 0, 0, 0);
  free (reads);
  return rc;
}

typedef struct { int *badList, *nBad, *lBad; } OvlMarkBad;
static void ovlMarkBadEach (void *v, U32 ix, const MgOvlRec *recs, U64 n)      /* modasm.c:1283-1289 */
{
  OvlMarkBad *b = (OvlMarkBad *) v;
  for (U64 i = 0 ; i < n ; ++i)
    if (recs[i].nBadFlip || recs[i].nBadOrder)
      { const U32 iy = recs[i].iy;
        ++b->nBad[iy];
        if (b->nBad[iy] < 10 && b->lBad[ix] < 10) b->badList[10 * (size_t) ix + b->lBad[ix]++] = (int) iy;
      }
}
static void ovlDropBad (const MgReadset *rs, OvlMarkBad *b)          /* modasm.c:1299-1302 */
{
  for (int ix = 1 ; ix <= rs->nReads ; ++ix)
    for (int i = b->lBad[ix] ; i-- ; )
      if (rs->bad[b->badList[10 * (size_t) ix + i]]) b->badList[10 * (size_t) ix + i] = b->badList[10 * (size_t) ix + --b->lBad[ix]];
}

int mgReadsetMarkBadReads (MgReadset *rs, FILE *out)                /* modasm.c:1266-1322 */
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  const int n = rs->nReads;
  memset (rs->bad, 0, (size_t) n + 1);
  OvlMarkBad b;
  b.badList = (int *) calloc (((size_t) n + 1) * 10, sizeof (int)); b.nBad = (int *) calloc ((size_t) n + 1, sizeof (int)); b.lBad = (int *) calloc ((size_t) n + 1, sizeof (int));
  U32 *reads = (U32 *) malloc (((size_t) n + 1) * sizeof (U32));
  for (int i = 0 ; i < n ; ++i) reads[i] = (U32) i + 1;
  const int rc = ovlDrive (rs, reads, (U32) n, 0, 0, 0, ovlMarkBadEach, &b);
  free (reads);
  if (!rc)
    { int N = 0;
      for (int ix = 1 ; ix <= n ; ++ix) if (b.nBad[ix] >= 10) { rs->bad[ix] |= BAD_ORDER10; ++N; b.lBad[ix] = 0; }
      if (out) fprintf (out, "MB  %d with >=10 bad overlaps\n", N);
      ovlDropBad (rs, &b);
      N = 0;
      for (int ix = 1 ; ix <= n ; ++ix) if (b.lBad[ix] >= 2) { rs->bad[ix] |= BAD_ORDER1; ++N; b.lBad[ix] = 0; }
      if (out) fprintf (out, "MB  %d with multiple bad overlaps\n", N);
      ovlDropBad (rs, &b);
      N = 0;
      for (int ix = 1 ; ix <= n ; ++ix) if (b.lBad[ix] > 0) { rs->bad[ix] |= BAD_ORDER1; ++N; b.lBad[ix] = 0; }
      if (out) fprintf (out, "MB  %d with single bad overlaps\n", N);
    }
  free (b.badList); free (b.nBad); free (b.lBad);
  return rc;
}

typedef struct { MgReadset *rs; } OvlContained;
static void ovlContainedEach (void *v, U32 ix, const MgOvlRec *recs, U64 n)    /* modasm.c:1382-1389 */
{
  MgReadset *rs = ((OvlContained *) v)->rs;
  int maxHit = 0;
  for (U64 i = 0 ; i < n ; ++i)
    { if (recs[i].iy == ix) continue;
      if (!(recs[i].flags & OVL_CONTAINED) || (int) recs[i].nHit <= maxHit) continue;
      rs->contained[ix] = (int) recs[i].iy; maxHit = recs[i].nHit;
    }
}

int mgReadsetMarkContained (MgReadset *rs, FILE *out)               /* modasm.c:1370-1394 */
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  const int n = rs->nReads;
  /* a read that is bad when its turn comes is not looked at (modasm.c:1380); a read's own flags are only ever set by its own turn, so which reads
     those are is known now */
  U32 *reads = (U32 *) calloc ((size_t) n + 1, sizeof (U32)); U32 nq = 0;
  for (int i = 1 ; i <= n ; ++i) if (!rs->bad[i]) reads[nq++] = (U32) i;
  OvlContained c; c.rs = rs;
  const int rc = ovlDrive (rs, reads, nq, 0, 0, 0, ovlContainedEach, &c);
  if (!rc)
    { int nContained = 0, nNot = 0; U64 totLen = 0;
      for (U32 q = 0 ; q < nq ; ++q) { const U32 ix = reads[q]; if (rs->contained[ix]) ++nContained; else { ++nNot; totLen += (U64) rs->len[ix]; } }
      if (out) fprintf (out, "MC  found %d contained reads, leaving %d not contained, av length %.1f\n", nContained, nNot, nNot ? totLen / (double) nNot : 0.);
    }
  free (reads);
  return rc;
}
