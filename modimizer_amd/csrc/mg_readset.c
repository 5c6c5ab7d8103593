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
#include <pthread.h>
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

static void rdnaForget (const MgReadset *rs);                       /* ModInfo, otherFlags and the -T count kept beside the set: at the end of this file */
static U8 *rdnaFlagsOf (const MgReadset *rs, int create);

void mgReadsetDestroy (MgReadset *rs)
{
  if (!rs) return;
  free (rs->len); free (rs->nHit); free (rs->nMiss); free (rs->nCopy); free (rs->hitStart); free (rs->bad); free (rs->contained);
  mgReadsetDevForget (rs); rdnaForget (rs);
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
  const U8 *other = rdnaFlagsOf (rs, 0);                              /* Read.otherFlags (modasm.c:47-53): set by -R, zero otherwise */
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { recs[i].otherFlags = other ? other[i] : 0;
      recs[i].len = rs->len[i]; recs[i].nHit = rs->nHit[i]; recs[i].nMiss = rs->nMiss[i];
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
  { int any = 0;
    for (int i = 1 ; i <= rs->nReads ; ++i) any |= recs[i].otherFlags;
    if (any) { U8 *other = rdnaFlagsOf (rs, 1); for (int i = 1 ; i <= rs->nReads ; ++i) other[i] = recs[i].otherFlags; }
  }
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

/* ---- modasm -R / -T / -rb: refFlag (modasm.c:752-860), testMods (595-748), resetBits (864-908) ----
 * ModInfo, the reads' otherFlags and the reference's static RUN are kept beside the set, keyed by its address (MgReadset's layout is pinned), and go with
 * mgReadsetDestroy.  Every pass works on copies of info[] and ModInfo and commits them when nothing can fail any more: on -1 nothing is modified. */

typedef struct RdnaState { const MgReadset *rs; MgModInfo *mi; size_t nMi; U8 *flags; int capFlags, run; struct RdnaState *next; } RdnaState;
static pthread_mutex_t gRdnaLock = PTHREAD_MUTEX_INITIALIZER;
static RdnaState *gRdna;
static __thread int gRdnaPath = -1;
static __thread U64 gRdnaDiag[4];
int mgReadsetRdnaPath (void) { return gRdnaPath; }
void mgReadsetRdnaDiag (U64 out4[4]) { memcpy (out4, gRdnaDiag, sizeof (gRdnaDiag)); }

static RdnaState *rdnaState (const MgReadset *rs, int create)
{
  pthread_mutex_lock (&gRdnaLock);
  RdnaState *s = gRdna;
  while (s && s->rs != rs) s = s->next;
  if (!s && create) { s = (RdnaState *) calloc (1, sizeof (RdnaState)); s->rs = rs; s->next = gRdna; gRdna = s; }
  pthread_mutex_unlock (&gRdnaLock);
  return s;
}
static void rdnaForget (const MgReadset *rs)
{
  pthread_mutex_lock (&gRdnaLock);
  for (RdnaState **p = &gRdna ; *p ; p = &(*p)->next)
    if ((*p)->rs == rs) { RdnaState *s = *p; *p = s->next; free (s->mi); free (s->flags); free (s); break; }
  pthread_mutex_unlock (&gRdnaLock);
}
/* otherFlags[0 .. nReads], zero for the reads that came since it was last asked for */
static U8 *rdnaFlags (RdnaState *s, const MgReadset *rs)
{
  if (s->capFlags < rs->nReads + 1)
    { s->flags = (U8 *) realloc (s->flags, (size_t) rs->nReads + 1);
      memset (s->flags + s->capFlags, 0, (size_t) (rs->nReads + 1 - s->capFlags));
      s->capFlags = rs->nReads + 1;
    }
  return s->flags;
}
const MgModInfo *mgReadsetModInfo (const MgReadset *rs) { RdnaState *s = rdnaState (rs, 0); return s ? s->mi : 0; }
static U8 *rdnaFlagsOf (const MgReadset *rs, int create) { RdnaState *s = rdnaState (rs, create); return s ? rdnaFlags (s, rs) : 0; }
const U8 *mgReadsetReadFlags (const MgReadset *rs) { return rdnaFlagsOf (rs, 1); }
int mgReadsetTestModsRun (const MgReadset *rs) { RdnaState *s = rdnaState (rs, 0); return s ? s->run : 0; }

#define MG_RDNA_DEVICE_MIN ((U64) 1 << 21)
enum { RD_REF = 1, RD_CORE = 2, RD_VAR = 4, RD_MULTI = 8 };        /* modasm.c:61-70 */
static U8 rdnaDepthClass (int depth) { return depth > 4750 ? RD_MULTI : depth > 2750 ? RD_CORE : RD_VAR; }      /* modasm.c:770-772,821-823 */

/* invBuild's nCopy[] (modasm.c:273-277) from info[] as it is going to be, into nc[(nReads + 1) * 4]: the device code of -C, or the loop */
static int rdnaTallies (const MgReadset *rs, const U8 *info, int host, int *nc)
{
  if (!host)
    { const int rc = mgReadsetCopyTallyDevice (rs->hit, rs->totHit, rs->hitStart, (U32) rs->nReads, info, rs->ms->max, nc);
      if (rc < 0) return -1;
      host = rc;
    }
  if (host)
    for (int r = 1 ; r <= rs->nReads ; ++r)
      { int *c = nc + 4 * (size_t) r; c[0] = c[1] = c[2] = c[3] = 0;
        for (U64 h = rs->hitStart[r] ; h < rs->hitStart[r + 1] ; ++h) ++c[info[rs->hit[h] & TOPMASK] & 3];
      }
  return 0;
}

static void rdnaN200Host (const MgReadset *rs, const U8 *qual, int *n200, int *m200)      /* modasm.c:781-802 */
{
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { const U32 *hit = rs->hit + rs->hitStart[i];
      const int nHit = (int) (rs->hitStart[i + 1] - rs->hitStart[i]);
      int n = 0; n200[i] = m200[i] = 0;
      for (int j = 0 ; j < nHit ; ++j) if (qual[hit[j] & TOPMASK] && ++n == 200) { n200[i] = j; break; }
      if (!n200[i]) continue;
      n = 0;
      for (int j = nHit ; --j ; ) if (qual[hit[j] & TOPMASK] && ++n == 200) { m200[i] = j; break; }
    }
}

int mgReadsetRefFlagHits (MgReadset *rs, const U32 *index, const int *pos, U64 n, FILE *out)
{
  gRdnaPath = -1;
  Modset *ms = rs->ms;
  if (modsetSyncToHost (ms, 0)) return -1;
  const size_t m = (size_t) ms->max + 1;
  for (U64 j = 0 ; j < n ; ++j)
    if (!index[j] || index[j] > ms->max) { char msg[160]; snprintf (msg, sizeof (msg), "-R: hit %llu names mod %u, the set holds 1 .. %u", (unsigned long long) j, index[j], ms->max); mgSetErrorText (msg); return -1; }
  RdnaState *s = rdnaState (rs, 1);
  if (s->mi && s->nMi != m) { mgSetErrorText ("-R: the modset has changed its size since the first -R"); return -1; }
  MgModInfo *mi = (MgModInfo *) calloc (m, sizeof (MgModInfo));
  U8 *info = (U8 *) malloc (m), *qual = (U8 *) malloc (m);
  int *n200 = (int *) calloc ((size_t) rs->nReads + 1, sizeof (int)), *m200 = (int *) calloc ((size_t) rs->nReads + 1, sizeof (int)), *rCount = (int *) calloc (m, sizeof (int));
  if (!mi || !info || !qual || !n200 || !m200 || !rCount) { free (mi); free (info); free (qual); free (n200); free (m200); free (rCount); mgSetErrorText ("-R: out of memory"); return -1; }
  if (s->mi) memcpy (mi, s->mi, m * sizeof (MgModInfo));
  memcpy (info, ms->info, m);
  for (U64 j = 0 ; j < n ; ++j)                                      /* modasm.c:766-773: the last hit of a mod wins rDNApos; bits are only ever set */
    { const U32 ix = index[j];
      info[ix] |= MS_RDNA;
      mi[ix].flags |= RD_REF | rdnaDepthClass (ms->depth[ix]); mi[ix].rDNApos = pos[j];
    }
  for (size_t i = 0 ; i < m ; ++i) qual[i] = (mi[i].flags & (RD_REF | RD_CORE)) == (RD_REF | RD_CORE);      /* fixed from here on: the walk below never sets RD_REF */
  int host = rsHostForced (rs);
  if (!host)
    { const int rc = mgRdnaN200Device (ms->max, qual, rs->hit, rs->totHit, rs->hitStart, (U32) rs->nReads, n200, m200);
      if (rc < 0) { free (mi); free (info); free (qual); free (n200); free (m200); free (rCount); return -1; }
      host = rc;
    }
  if (host) rdnaN200Host (rs, qual, n200, m200);
  U8 *flags = rdnaFlags (s, rs);
  int nRDNAreads = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i)                            /* modasm.c:803-830, in read order: running averages, mods newly flagged by earlier reads */
    { if (m200[i] <= n200[i]) continue;
      const U32 *hit = rs->hit + rs->hitStart[i];
      int lastPos = 0;
      for (int j = n200[i] ; j < m200[i] ; ++j)
        { const U32 h = hit[j] & TOPMASK;
          MgModInfo *q = &mi[h];
          if (q->flags)
            { const int p = q->rDNApos;
              if (q->flags & RD_REF) lastPos = p;
              else if (p > 0 && p < lastPos + 50 && p > lastPos - 50) { q->rDNApos = (rCount[h] * p + lastPos) / (rCount[h] + 1); ++rCount[h]; }
              else q->rDNApos = -1;
            }
          else
            { info[h] |= MS_RDNA; q->flags |= rdnaDepthClass (ms->depth[h]); q->rDNApos = lastPos; rCount[h] = 1; }
        }
      flags[i] |= 1; ++nRDNAreads;
    }
  free (s->mi); s->mi = mi; s->nMi = m;
  memcpy (ms->info, info, m);
  mgModsetHostChanged (ms);
  gRdnaPath = host;
  int nRDNA = 0, nRef = 0, nGoodPos = 0, nRefC = 0, nRefV0 = 0, nRefV1 = 0, nRefM = 0, nOthC = 0, nOthV0 = 0, nOthV1 = 0, nOthM = 0;      /* modasm.c:834-859 */
  for (size_t i = 0 ; i < m ; ++i)
    { const MgModInfo *q = &mi[i];
      if (!q->flags) continue;
      ++nRDNA;
      const int copy0 = (info[i] & 3) == 0;
      if (q->flags & RD_REF)
        { ++nRef;
          if (q->flags & RD_CORE) ++nRefC; else if (q->flags & RD_MULTI) ++nRefM; else if (copy0) ++nRefV0; else ++nRefV1;
        }
      else
        { if (q->flags & RD_CORE) ++nOthC; else if (q->flags & RD_MULTI) ++nOthM; else if (copy0) ++nOthV0; else ++nOthV1;
          if (q->rDNApos > 0) ++nGoodPos;
        }
    }
  if (out)
    { fprintf (out, "total nRDNAreads %d other reads %d\n", nRDNAreads, rs->nReads - nRDNAreads);
      fprintf (out, "total nRDNAmods %d nRDNAref %d other mods %d\n", nRDNA, nRef, (int) m - nRDNA);
      fprintf (out, "  nRefC %d nRefM %d nRefVcopy>0 %d nRefVcopy0 %d\n", nRefC, nRefM, nRefV1, nRefV0);
      fprintf (out, "  nOthC %d nOthM %d nOthVcopy>0 %d nOthVcopy0 %d", nOthC, nOthM, nOthV1, nOthV0);
      fprintf (out, " nGoodPos %d\n", nGoodPos);
    }
  free (info); free (qual); free (n200); free (m200); free (rCount);
  return 0;
}

/* the reference sequences' hits in file order: scan with the set's hasher and lookups on the device, as mgRefPaintFile makes them (misses dropped here) */
typedef struct { Modset *ms; U32 *ix; int *pos; U64 n, cap; MgSeedBufs bufs; } RefHitsCtx;
static int refHitsDeviceBatch (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, void *stream)
{
  RefHitsCtx *c = (RefHitsCtx *) v; (void) idBytes; (void) idOff; (void) stream;
  if (!nReads) return 0;
  U64 n = 0;
  if (mgSeedsOfBatch (c->ms, 0, 0, dPacked, total, dOff, nReads, mgSeedGuess (c->ms->hasher->w, total), &c->bufs, &n, 0)) return -1;
  if (!n) return 0;
  U32 *ix = (U32 *) malloc (n * sizeof (U32)), *pf = (U32 *) malloc (n * sizeof (U32));
  int rc = !ix || !pf || mgMemcpyD2H (ix, c->bufs.ix, n * sizeof (U32), 0) || mgMemcpyD2H (pf, c->bufs.posF, n * sizeof (U32), 0) ? -1 : 0;
  if (!rc && c->n + n > c->cap)
    { c->cap = (c->n + n) * 2; c->ix = (U32 *) realloc (c->ix, c->cap * sizeof (U32)); c->pos = (int *) realloc (c->pos, c->cap * sizeof (int));
      if (!c->ix || !c->pos) rc = -1;
    }
  for (U64 j = 0 ; !rc && j < n ; ++j) if (ix[j]) { c->ix[c->n] = ix[j]; c->pos[c->n++] = (int) (pf[j] & MG_POS_MASK); }
  free (ix); free (pf);
  return rc;
}
static int refHitsHostBatch (MgSeqBatch *b, void *v)
{
  if (b->nSeq <= 0) return 0;
  MgDevBatch d; mgBatchUpload (&d, b->bases, b->offsets, b->nSeq);
  const int rc = refHitsDeviceBatch (v, (const U32 *) d.dPacked, d.total, (const U64 *) d.dOff, (U32) b->nSeq, 0, 0, 0);
  mgBatchFree (&d);
  return rc;
}

int mgReadsetRefFlagFile (MgReadset *rs, const char *refFile, FILE *out)      /* modasm.c:752-776, then the above */
{
  gRdnaPath = -1;
  { FILE *f = fopen (refFile, "rb");
    if (!f) { char msg[600]; snprintf (msg, sizeof (msg), "failed to open ref seq file %s", refFile); mgSetErrorText (msg); return -1; }      /* modasm.c:756 */
    fclose (f);
  }
  if (mgIterRequireDevice ()) return -1;
  RefHitsCtx c; memset (&c, 0, sizeof (c)); c.ms = rs->ms;
  U64 nSeq = 0, totLen = 0, resumeOff = 0, resumeLine = 1;
  int rc = mgTextForEachBatchDevice (refFile, refHitsDeviceBatch, &c, 0, 0, &nSeq, &totLen, &resumeOff, &resumeLine);
  if (rc == -2) rc = mgSeqForEachBatchFrom (refFile, 0, 1, 0, refHitsHostBatch, &c);
  else if (rc == -3) rc = mgSeqForEachBatchFrom (refFile, (size_t) resumeOff, resumeLine, nSeq, refHitsHostBatch, &c);
  mgSeedBufsFree (&c.bufs);
  if (rc) { if (!mgLastError ()[0]) mgSetErrorText ("-R: failed to read the reference sequence file"); rc = -1; }
  else rc = mgReadsetRefFlagHits (rs, c.ix, c.pos, c.n, out);
  free (c.ix); free (c.pos);
  return rc;
}

int mgReadsetResetBits (MgReadset *rs, int op, FILE *out)          /* modasm.c:864-908 */
{
  gRdnaPath = -1;
  Modset *ms = rs->ms;
  RdnaState *s = rdnaState (rs, 0);
  if (!s || !s->mi) { mgSetErrorText ("-rb: need to run -R first (the reference reads a null ModInfo)"); return -1; }
  if (modsetSyncToHost (ms, 0)) return -1;
  const size_t m = (size_t) ms->max + 1;
  if (s->nMi != m) { mgSetErrorText ("-rb: the modset has changed its size since -R"); return -1; }
  if (op == 3 && rs->nReads < 1) { mgSetErrorText ("-rb 3: the read set is empty (the reference reads read 1)"); return -1; }
  U8 *info = (U8 *) malloc (m);
  int *nc = (int *) calloc (((size_t) rs->nReads + 1) * 4, sizeof (int));
  if (!info || !nc) { free (info); free (nc); mgSetErrorText ("-rb: out of memory"); return -1; }
  memcpy (info, ms->info, m);
  int n = 0;
  const char *line = 0;
  if (op >= 1 && op <= 3)
    { for (size_t i = 0 ; i < m ; ++i)
        if ((s->mi[i].flags & RD_CORE) && !(op == 2 && (info[i] & MS_REPEAT))) { info[i] = (U8) ((info[i] & 0xfc) | 1); ++n; }
        else info[i] &= 0xfc;
      line = op == 1 ? "resetting rDNA core kmers to copy1, rest to copy0:" : op == 2 ? "resetting non-repetitive rDNA core kmers to copy1, rest to copy0:"
                     : "resetting rDNA core kmers not repeated in read 1 to copy1: ";
    }
  if (op == 3)
    { U8 *z = (U8 *) calloc (m, 1);
      for (U64 h = rs->hitStart[1] ; h < rs->hitStart[2] ; ++h)
        { const U32 y = rs->hit[h] & TOPMASK;
          if ((info[y] & 3) != 1) continue;
          if (z[y]) { info[y] &= 0xfc; --n; } else z[y] = 1;
        }
      free (z);
    }
  const int host = rsHostForced (rs);
  if (rdnaTallies (rs, info, host, nc)) { free (info); free (nc); return -1; }      /* invBuild (modasm.c:907): depth[] is as it was, so only nCopy[] moves */
  memcpy (ms->info, info, m);
  if (rs->nReads) memcpy (rs->nCopy[1], nc + 4, (size_t) rs->nReads * sizeof (int[4]));
  mgModsetHostChanged (ms);
  gRdnaPath = host;
  if (line && out) fprintf (out, "%s %d kept\n", line, n);
  free (info); free (nc);
  return 0;
}

/* testMods' gather and rules by loops: per tested mod the count / least / greatest distance per partner in arrays of ms->max + 1 entries that are
   stamped with the tested mod's ordinal, not cleared.  0, or -2 with *badMod where the reference breaks */
static int rdnaTestModsHost (const MgRdnaSet *S, const U32 *tested, U32 nTested, int wantCells, int *res3, int *badLD, int *splitLD, U64 *cellStart, MgLdCell **cellsOut,
                             U64 diag[4], U32 *badMod)
{
  const size_t m = (size_t) S->msMax + 1;
  int maxLen = 0;
  for (U32 r = 1 ; r <= S->nReads ; ++r) if (S->len[r] > maxLen) maxLen = S->len[r];
  int *pos = (int *) malloc ((S->totHit + 1) * sizeof (int));
  for (U32 r = 1 ; r <= S->nReads ; ++r) { int x = 0; for (U64 h = S->hitStart[r] ; h < S->hitStart[r + 1] ; ++h) pos[h] = x += S->dx[h]; }
  U32 *stamp = (U32 *) calloc (m, sizeof (U32)), *touched = (U32 *) malloc (m * sizeof (U32));
  int *cnt = (int *) malloc (m * sizeof (int)), *mn = (int *) malloc (m * sizeof (int)), *mx = (int *) malloc (m * sizeof (int));
  int *start = (int *) calloc ((size_t) maxLen + 2, sizeof (int)), *end = (int *) calloc ((size_t) maxLen + 2, sizeof (int));
  MgLdCell *cells = 0; U64 nCells = 0, capCells = 0;
  int rc = 0, nBigS = 0, nBigE = 0;
  for (U32 t = 0 ; t < nTested && !rc ; ++t)
    { const U32 i = tested[t];
      int extS = 0, extE = 0; U32 nTouched = 0;
      for (U64 v = S->invStart[i] ; v < S->invStart[i + 1] && !rc ; ++v)
        { const U32 r = S->invSpace[v];
          const U64 h0 = S->hitStart[r], h1 = S->hitStart[r + 1];
          U64 f = h0;
          while (f < h1 && (S->hit[f] & TOPMASK) != i) ++f;            /* both visits of a read that holds i twice use the first occurrence */
          const int x = f < h1 ? pos[f] : 0, o = S->len[r] - x - S->w;
          if (f == h1 || o < 0 || x > maxLen || o > maxLen) { rc = -2; *badMod = i; break; }
          const int fwd = (S->hit[f] & TOPBIT) != 0, s = fwd ? x : o, e = fwd ? o : x;
          ++start[s]; ++end[e];
          if (s + 1 > extS) extS = s + 1;
          if (e + 1 > extE) extE = e + 1;
          for (U64 h = h0 ; h < h1 ; ++h)
            { const U32 y = S->hit[h] & TOPMASK;
              if (h == f || !mgRdnaCheckMod (S->info[y])) continue;
              const int d = fwd ? pos[h] - x : x - pos[h];
              if (stamp[y] != t + 1) { stamp[y] = t + 1; touched[nTouched++] = y; cnt[y] = 0; mn[y] = mx[y] = d; }
              ++cnt[y];
              if (d < mn[y]) mn[y] = d;
              if (d > mx[y]) mx[y] = d;
            }
        }
      if (!rc && ((extS > MG_RDNA_CLEARED && ++nBigS > 1) || (extE > MG_RDNA_CLEARED && ++nBigE > 1))) { rc = -3; *badMod = i; }
      if (!rc)
        { for (int k = extS - 1 ; k-- > 0 ; ) start[k] += start[k + 1];      /* modasm.c:651-654 */
          for (int k = extE - 1 ; k-- > 0 ; ) end[k] += end[k + 1];
          qsort (touched, nTouched, sizeof (U32), rsU32Cmp);
          if (wantCells && nCells + nTouched > capCells) { capCells = (nCells + nTouched) * 2 + 64; cells = (MgLdCell *) realloc (cells, capCells * sizeof (MgLdCell)); }
          for (U32 q = 0 ; q < nTouched ; ++q)
            { const U32 y = touched[q];
              MgLdCell c; c.m = y;
              if (mgRdnaLdRule (cnt[y], mn[y], mx[y], start, extS, end, extE, (int) S->depth[y], S->run, &c)) { rc = -2; *badMod = i; break; }
              diag[3] += (U64) cnt[y];
              if (c.flags & MG_LD_GOOD) ++res3[3 * (size_t) t];
              if (c.flags & MG_LD_MOD2) ++res3[3 * (size_t) t + 1];
              if (c.flags & MG_LD_SPLIT) { ++res3[3 * (size_t) t + 2]; ++splitLD[y]; }
              if (c.flags & MG_LD_BAD_M) ++badLD[y];
              if (c.flags & MG_LD_BAD_I) ++badLD[i];
              if (wantCells) cells[nCells++] = c;
            }
          if (cellStart) cellStart[t + 1] = wantCells ? nCells : 0;
        }
      memset (start, 0, (size_t) (extS > 0 ? extS : 1) * sizeof (int)); memset (end, 0, (size_t) (extE > 0 ? extE : 1) * sizeof (int));
    }
  free (pos); free (stamp); free (touched); free (cnt); free (mn); free (mx); free (start); free (end);
  if (rc) { free (cells); return rc; }
  diag[0] = nTested ? 1 : 0;
  *cellsOut = cells;
  return 0;
}

/* the closing loop of testMods (modasm.c:708-740) over ModInfo: the copy-0 resets into info[], the "YY-TEST" lines into yFile (0: none); the misleading
   braces at RUN 4 and 8 -- "BADLD" printed for, and copy 0 given to, EVERY mod -- are kept */
static void rdnaTestModsClose (const MgModInfo *mi, size_t m, const U16 *depth, U8 *info, int run, FILE *yFile, int zero[3])
{
  zero[0] = zero[1] = zero[2] = 0;
  for (size_t i = 0 ; i < m ; ++i)
    { const MgModInfo *q = &mi[i];
      const int d = depth[i];
#define RD_BADLD() do { if (yFile) fprintf (yFile, "BADLD %d depth %d nBadLD %d nSplitLD %d\n", (int) i, d, q->nBadLD, q->nSplitLD); info[i] &= 0xfc; ++zero[2]; } while (0)
      if ((q->nGood || q->nMod2) && yFile) fprintf (yFile, "TEST %d depth %d nGood %d nMod2 %d nBadLD %d nSplit %d\n", (int) i, d, q->nGood, q->nMod2, q->nBadLD, q->nSplit);
      if (q->nGood < q->nMod2) { info[i] &= 0xfc; ++zero[0]; }
      if (q->nSplit > 10) { info[i] &= 0xfc; ++zero[1]; }
      if ((run == 2 || run == 6) && (q->nBadLD > 20 || q->nSplitLD > 10)) RD_BADLD ();
      if (run == 3 || run == 7)
        { if (q->nMod2 > 25) { info[i] &= 0xfc; ++zero[0]; }
          if (q->nSplit) { info[i] &= 0xfc; ++zero[1]; }
          if (q->nBadLD > 10) RD_BADLD ();
        }
      if (run == 4 || run == 8)
        { if (q->nBadLD > 6 && q->nSplit) { info[i] &= 0xfc; ++zero[1]; }
          RD_BADLD ();
        }
#undef RD_BADLD
    }
}

int mgReadsetTestMods (MgReadset *rs, int minDepth, int maxDepth, FILE *yFile, FILE *zFile, FILE *out)      /* modasm.c:595-748 */
{
  gRdnaPath = -1; memset (gRdnaDiag, 0, sizeof (gRdnaDiag));
  Modset *ms = rs->ms;
  RdnaState *s = rdnaState (rs, 0);
  if (!s || !s->mi) { mgSetErrorText ("need to run -R first"); return -1; }      /* modasm.c:609 */
  if (modsetSyncToHost (ms, 0)) return -1;
  const size_t m = (size_t) ms->max + 1;
  char msg[240];
  if (s->nMi != m) { mgSetErrorText ("-T: the modset has changed its size since -R"); return -1; }
  if (!rs->invStart || !rs->invSpace) { mgSetErrorText ("-T: the read set has no inverse lists (nothing was read into it)"); return -1; }
  if (rs->invStart[m] > rs->totHit) { mgSetErrorText ("-T: the depths of the mods add up to more than the hits of the reads: the inverse lists do not fit (modasm.c:265-270)"); return -1; }
  U32 *tested = (U32 *) malloc (m * sizeof (U32)), *partner = (U32 *) malloc (m * sizeof (U32));
  U32 nTested = 0, nPartner = 0; U64 visits = 0, walked = 0;      /* walked: the hits of the visited reads, a bound of the partner occurrences */
  int rc = 0;
  for (size_t i = 0 ; i < m && !rc ; ++i)                            /* modasm.c:614-615; the partners are the mods that pass checkMod */
    { if (!mgRdnaCheckMod (ms->info[i])) continue;
      partner[nPartner++] = (U32) i;
      const int d = ms->depth[i];
      if (d < minDepth || d >= maxDepth) continue;
      const U64 a = rs->invStart[i], e = rs->invStart[i + 1];
      if (d == 0 || d == 0xffff || e - a != (U64) d || e > rs->totHit)
        { snprintf (msg, sizeof (msg), "-T: tested mod %u has depth %d and a list of %llu reads (a mod of depth 0 or 65535 has no list: modasm.c:266,617)", (U32) i, d, (unsigned long long) (e - a));
          mgSetErrorText (msg); rc = -1; break; }
      for (U64 v = a ; v < e ; ++v)
        { if (rs->invSpace[v] < 1 || rs->invSpace[v] > (U32) rs->nReads) { mgSetErrorText ("-T: an inverse list names a read that is not in the set"); rc = -1; break; }
          walked += rs->hitStart[rs->invSpace[v] + 1] - rs->hitStart[rs->invSpace[v]];
        }
      tested[nTested++] = (U32) i; visits += e - a;
    }
  if (!rc && !nTested) { mgSetErrorText ("-T: no mod tested (the reference dies at the end of such a call: arrayDestroy (0), modasm.c:746)"); rc = -1; }
  const int run = s->run + 1;
  int *res3 =(int *) calloc ((size_t) nTested * 3 + 1, sizeof (int)), *badLD = (int *) calloc (m, sizeof (int)), *splitLD = (int *) calloc (m, sizeof (int));
  U64 *cellStart = (U64 *) calloc ((size_t) nTested + 2, sizeof (U64));
  MgLdCell *cells = 0;
  MgModInfo *mi = (MgModInfo *) malloc (m * sizeof (MgModInfo));
  U8 *info = (U8 *) malloc (m);
  int *nc = (int *) calloc (((size_t) rs->nReads + 1) * 4, sizeof (int));
  /* a call that walks fewer than MG_RDNA_DEVICE_MIN hits is done by the host loops before the set's arrays have reached the device (2.3 ms
     against 1.6 ms at 2 x 10^4 occurrences, 2.8 ms against 100 ms at 10^8); MODGPU_READSET_HOST=0 sends every call to the device */
  int host = rsHostForced (rs) || (walked < MG_RDNA_DEVICE_MIN && mgKnobs ()->readsetHost != 0);
  U32 badMod = 0;
  if (!rc)
    { MgRdnaSet S; S.msMax = ms->max; S.w = ms->hasher->w; S.run = run; S.info = ms->info; S.depth = ms->depth; S.hit = rs->hit; S.dx = rs->dx; S.totHit = rs->totHit;
      S.hitStart = rs->hitStart; S.len = rs->len; S.nReads = (U32) rs->nReads; S.invStart = rs->invStart; S.invSpace = rs->invSpace;
      const MgKnobs *kn = mgKnobs ();
      const U32 batch = kn->testModsBatch != MG_KNOB_UNSET && kn->testModsBatch > 0 ? (U32) kn->testModsBatch : 0;
      if (!host)
        { rc = mgRdnaTestModsDevice (&S, tested, nTested, partner, nPartner, batch, zFile != 0, res3, badLD, splitLD, cellStart, &cells, gRdnaDiag, &badMod);
          if (rc == 1) { host = 1; rc = 0; memset (res3, 0, ((size_t) nTested * 3 + 1) * sizeof (int)); memset (badLD, 0, m * sizeof (int)); memset (splitLD, 0, m * sizeof (int)); memset (gRdnaDiag, 0, sizeof (gRdnaDiag)); }
        }
      if (host && !rc) rc = rdnaTestModsHost (&S, tested, nTested, zFile != 0, res3, badLD, splitLD, cellStart, &cells, gRdnaDiag, &badMod);
      if (rc == -2)
        { snprintf (msg, sizeof (msg), "-T: tested mod %u: a visit counts before its array (len - x - w < 0) or a distance is looked up beyond it (modasm.c:630,664,689); w > k?", badMod);
          mgSetErrorText (msg); rc = -1; }
      if (rc == -3)
        { snprintf (msg, sizeof (msg), "-T: tested mod %u is the second whose count array passes 20000 cells: the reference clears only the first 20000 between tested mods and counts on stale cells (modasm.c:619-620, array.c:103)", badMod);
          mgSetErrorText (msg); rc = -1; }
    }
  int zero[3];
  if (!rc)
    { memcpy (mi, s->mi, m * sizeof (MgModInfo)); memcpy (info, ms->info, m);
      for (size_t i = 0 ; i < m ; ++i) { mi[i].nGood = mi[i].nMod2 = mi[i].nSplit = 0; mi[i].nBadLD = badLD[i]; mi[i].nSplitLD = splitLD[i]; }      /* modasm.c:610-611 */
      for (U32 t = 0 ; t < nTested ; ++t) { MgModInfo *q = &mi[tested[t]]; q->nGood = res3[3 * (size_t) t]; q->nMod2 = res3[3 * (size_t) t + 1]; q->nSplit = res3[3 * (size_t) t + 2]; }
      rdnaTestModsClose (mi, m, ms->depth, info, run, 0, zero);
      if (rdnaTallies (rs, info, host, nc)) rc = -1;                 /* invBuild (modasm.c:744): nCopy[] after the copy-0 resets */
    }
  if (!rc)
    { if (zFile)
        for (U32 t = 0 ; t < nTested ; ++t)
          for (U64 c = cellStart[t] ; c < cellStart[t + 1] ; ++c)
            fprintf (zFile, "i %d depth %d m %d depth %d %c count %d min %d at %d max %d at %d\n", (int) tested[t], (int) ms->depth[tested[t]], (int) cells[c].m, (int) ms->depth[cells[c].m],
                     (cells[c].flags & MG_LD_PLUS) ? '+' : '-', cells[c].n, cells[c].vmin, cells[c].xmin, cells[c].vmax, cells[c].xmax);
      memcpy (info, ms->info, m);
      rdnaTestModsClose (mi, m, ms->depth, info, run, yFile, zero);
      memcpy (ms->info, info, m);
      { MgModInfo *old = s->mi; s->mi = mi; mi = old; }
      if (rs->nReads) memcpy (rs->nCopy[1], nc + 4, (size_t) rs->nReads * sizeof (int[4]));
      s->run = run;
      mgModsetHostChanged (ms);
      gRdnaPath = host; gRdnaDiag[1] = nTested; gRdnaDiag[2] = visits;
      if (out) fprintf (out, "RUN %d tested %d mods and zeroed %d bad>good %d split %d LD\n", run, (int) nTested, zero[0], zero[1], zero[2]);
    }
  free (tested); free (partner); free (res3); free (badLD); free (splitLD); free (cellStart); free (cells); free (mi); free (info); free (nc);
  return rc;
}
