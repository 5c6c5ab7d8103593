/* mg_seqfiles.c — the callers' file loops: a FASTA / FASTQ file into a set, a Reference, a query, a painted report.
 * Plain text, blocked gzip and ordinary gzip from MODGPU_GZIP_MIN_KB up are parsed on the device (mg_textgpu.hip) and handed on batch by batch; what
 * that parser leaves -- smaller gzip files, a last line without its newline (-2), FASTQ that breaks a rule, a gzip FASTA file whose last record is
 * unfinished (-3) -- goes through the host parser's batch loop
 * (mg_seqio.c), from the start or from the record the device parser stopped at.
 */
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "modgpu.h"
#include "mg_internal.h"

/* what a device walk that returned rc = -2 or -3 leaves to the host parser: on -2 the whole file, on -3 from byte resumeOff of its text (a record start, line
   resumeLine, nSeq records before it); every batch to hostFn.  Any other rc comes back as it is */
static int hostParserTakes (int rc, const char *filename, U64 resumeOff, U64 resumeLine, U64 nSeq, int (*hostFn) (MgSeqBatch *, void *), void *ctx)
{
  if (rc == -2) return mgSeqForEachBatchFrom (filename, 0, 1, 0, hostFn, ctx);
  if (rc == -3) return mgSeqForEachBatchFrom (filename, (size_t) resumeOff, resumeLine, nSeq, hostFn, ctx);
  return rc;
}

/* a host parser's batch for a callback that takes device batches: uploaded, its ids as one block and their offsets in it (the ids share one block:
   mgSeqBatchFree) */
typedef struct { MgTextBatchFn devFn; void *ctx; } WalkUpload;
static int walkUploadBatch (MgSeqBatch *b, void *v)
{
  WalkUpload *u = (WalkUpload *) v;
  if (b->nSeq <= 0) return 0;
  U64 *idOff = (U64 *) malloc ((size_t) b->nSeq * 8);
  if (!idOff) return -1;
  for (int r = 0 ; r < b->nSeq ; ++r) idOff[r] = (U64) (b->names[r] - b->names[0]);
  MgDevBatch d; mgBatchUpload (&d, b->bases, b->offsets, b->nSeq);
  const int rc = u->devFn (u->ctx, (const U32 *) d.dPacked, d.total, (const U64 *) d.dOff, (U32) b->nSeq, b->names[0], idOff, 0);
  mgBatchFree (&d);
  free (idOff);
  return rc;
}

/* plain FASTA / FASTQ text is parsed on the device (mg_textgpu.hip) and goes to devFn batch by batch; the rest of it by the host parser.  hostFn takes the
   host parser's batches, 0: each is uploaded and goes to devFn */
int mgSeqWalkFile (const char *filename, MgTextBatchFn devFn, int (*hostFn) (MgSeqBatch *, void *), void *ctx, U64 batchBases, U64 batchRecs, U64 *nSeq, U64 *totLen)
{
  WalkUpload u; u.devFn = devFn; u.ctx = ctx;
  void *hostCtx = hostFn ? ctx : (void *) &u;
  if (!hostFn) hostFn = walkUploadBatch;
  U64 resumeOff = 0, resumeLine = 1;
  const int rc = mgTextForEachBatchDevice (filename, devFn, ctx, batchBases, batchRecs, nSeq, totLen, &resumeOff, &resumeLine);
  return hostParserTakes (rc, filename, resumeOff, resumeLine, *nSeq, hostFn, hostCtx);
}

/* ---- modutils: a file into a set (modutils.c:33-51) ---- */

typedef struct { Modset *ms; U64 nSeq, totLen, totHash; } AddCtx;
static int addBatch (MgSeqBatch *b, void *v)
{
  AddCtx *c = (AddCtx *) v;
  int64_t h = mgAddSequenceBatch (c->ms, b->bases, b->offsets, b->nSeq);
  if (h < 0) return -1;
  c->nSeq += (U64) b->nSeq; c->totLen += (U64) b->total; c->totHash += (U64) h;
  return 0;
}

/* the host parser's legs of a 10x file: the batch's records go on from the file's count, so the odd ones stay the odd ones */
static int addBatch10x (MgSeqBatch *b, void *v)
{
  AddCtx *c = (AddCtx *) v;
  mgAdd10xDiagHostLeg ();
  int64_t h = mgAddSequenceBatch10x (c->ms, b->bases, b->offsets, b->nSeq, c->nSeq + 1);
  if (h < 0) return -1;
  c->nSeq += (U64) b->nSeq; c->totLen += (U64) b->total; c->totHash += (U64) h;
  return 0;
}

/* plain FASTA / FASTQ text: the device parses it (devFile: mg_textgpu.hip; a 10x file's batches are trimmed where they lie), the host only moves
   the bytes; everything else -- gzip, a last line without its newline, the rest of a FASTQ file that breaks a rule (a record that breaks the rules,
   an unfinished one: from the first record the device parser has not added) -- through the host parser and hostFn */
typedef int (*AddFileDeviceFn) (Modset *ms, const char *filename, U64 *nSeq, U64 *totLen, U64 *totHash, U64 *resumeOff, U64 *resumeLine);
static int addSequenceFile (Modset *ms, const char *filename, FILE *out, AddFileDeviceFn devFile, int (*hostFn) (MgSeqBatch *, void *))
{
  AddCtx c; memset (&c, 0, sizeof (c)); c.ms = ms;
  U64 resumeOff = 0, resumeLine = 1;
  int rc = devFile (ms, filename, &c.nSeq, &c.totLen, &c.totHash, &resumeOff, &resumeLine);
  if (rc == -1) return -1;
  rc = hostParserTakes (rc, filename, resumeOff, resumeLine, c.nSeq, hostFn, &c);
  if (rc) return rc;
  fprintf (out, "added %llu sequences total length %llu total hashes %llu, new max %u\n",
           (unsigned long long) c.nSeq, (unsigned long long) c.totLen, (unsigned long long) c.totHash, ms->max);
  return 0;
}

int mgAddSequenceFile (Modset *ms, const char *filename, FILE *out)            /* modutils.c:33-51 */
{ return addSequenceFile (ms, filename, out, mgAddSequenceFileDevice, addBatch); }

int mgAddSequenceFile10x (Modset *ms, const char *filename, FILE *out)         /* modutils.c:33-51 with is10x */
{
  mgAdd10xDiagReset ();
  return addSequenceFile (ms, filename, out, mgAddSequenceFile10xDevice, addBatch10x);
}

/* ---- modmap: the Reference's file ---- */

typedef struct { MgReference *ref; bool isAdd; } RefDevCtx;
static int refDeviceBatch (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, void *stream)
{
  RefDevCtx *c = (RefDevCtx *) v; (void) stream;
  const char **names = (const char **) malloc (((size_t) nReads + 1) * sizeof (char *));
  mgIdPointers (names, idBytes, idOff, nReads);
  int rc = mgReferenceAddDevice (c->ref, dPacked, total, dOff, (int) nReads, names, c->isAdd);
  free (names);
  return rc;
}

/* the end of a reference file that the device parser handed over at its last record (-3): the host parser's batches, uploaded, go where the device
   parser's went */
typedef struct { WalkUpload up; U64 total; } RefTailCtx;
static int refTailBatch (MgSeqBatch *b, void *v) { RefTailCtx *t = (RefTailCtx *) v; t->total += (U64) b->total; return walkUploadBatch (b, &t->up); }

/* modmap reads the whole reference before it classifies and packs (modmap.c:93-134), and its report
 * lines are per file.  Plain FASTA text is parsed on the device (mg_textgpu.hip), batch by batch -- first-occurrence
 * indices do not depend on where a stream is cut -- everything else by the host parser as one batch holding every record */
int mgReferenceFastaRead (MgReference *ref, const char *filename, bool isAdd, FILE *out)
{
  { RefDevCtx c; c.ref = ref; c.isAdd = isAdd;
    U64 nSeq = 0, totLen = 0, resumeOff = 0, resumeLine = 1;
    const int first = mgTextFirstByte (filename);        /* (of the text: a blocked-gzip file is looked into) */
    if (first == '>')                                     /* (a FASTQ reference goes the host way: the hand-over in the middle of a file is not worth having here) */
      { const int rc = mgTextForEachBatchDevice (filename, refDeviceBatch, &c, 0, 0, &nSeq, &totLen, &resumeOff, &resumeLine);
        if (rc == -1) return -1;
        if (rc == 0) { mgReferenceFinish (ref, totLen, isAdd, out); return 0; }
        if (rc == -3)                                     /* (ordinary gzip whose last record is unfinished: the records before it are in, the host parser says what the reference says about the last) */
          { RefTailCtx t; t.up.devFn = refDeviceBatch; t.up.ctx = &c; t.total = 0;
            if (hostParserTakes (-3, filename, resumeOff, resumeLine, nSeq, refTailBatch, &t)) return -1;
            mgReferenceFinish (ref, totLen + t.total, isAdd, out);
            return 0;
          }
      }
  }
  MgSeqReader *r = mgSeqOpen (filename);
  if (!r) { fprintf (stderr, "FATAL ERROR: failed to read reference sequence file %s\n", filename); exit (-1); }   /* modmap.c:99 */
  MgSeqBatch b;
  int n = mgSeqNextBatch (r, INT64_MAX, &b);
  int rc = mgReferenceRead (ref, b.bases, b.offsets, n, (const char **) b.names, isAdd, out);
  mgSeqBatchFree (&b);
  mgSeqClose (r);
  return rc;
}

/* ---- modmap: the query's file ---- */

typedef struct { MgReference *ref; FILE *out; } QueryCtx;
static int queryBatch (MgSeqBatch *b, void *v)
{ QueryCtx *c = (QueryCtx *) v; return mgQueryProcess (c->ref, b->bases, b->offsets, b->nSeq, (const char **) b->names, c->out); }

static int queryDeviceBatch (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, void *stream)
{ (void) stream; return mgQueryPipePush ((MgQueryPipe *) v, dPacked, total, dOff, (int) nReads, idBytes, idOff); }

/* short reads: a query batch per window of the file (128 MiB of text; a batch is handed on at the first window's end at which it holds
   this many bases and records): the lines of one batch are formatted and written while the next one is read, parsed and queried.
   Long reads (few lines): batches of the default size, 1 Gbp -- the chaining of a batch (mg_chain.hip) takes as long as the serial
   walk of its longest read, whatever else it holds: 38 batches of 134 Mbp spent 17 ms there per 5 Gbp */
#define MG_QUERY_FILE_BATCH 32000000ull
#define MG_QUERY_FILE_BATCH_RECS 200000ull

int mgQueryFile (MgReference *ref, const char *filename, FILE *out)            /* modmap.c:188-196 */
{
  QueryCtx c; c.ref = ref; c.out = out;
  /* plain FASTA / FASTQ text: parsed on the device, the batches stay there (no 1-byte-per-base upload); gzip, a last line without
     its newline, FASTQ that breaks a rule: the host parser (from the first record the device parser has not handed on) */
  U64 nSeq = 0, totLen = 0, resumeOff = 0, resumeLine = 1;
  MgQueryPipe *pipe = mgQueryPipeOpen (ref, out);
  int rc = mgTextForEachBatchDevice (filename, queryDeviceBatch, pipe, MG_QUERY_FILE_BATCH, MG_QUERY_FILE_BATCH_RECS, &nSeq, &totLen, &resumeOff, &resumeLine);
  mgQueryPipeClose (pipe);                                 /* every line of the device parser's batches is out */
  if (rc == 0 || rc == -1) return rc;
  const int whole = rc != -3;                              /* (-2, and whatever else the walk may return: the whole file) */
  rc = hostParserTakes (whole ? -2 : -3, filename, resumeOff, resumeLine, nSeq, queryBatch, &c);
  if (whole && rc == -1 && access (filename, R_OK)) { fprintf (stderr, "FATAL ERROR: failed to read query sequence file %s\n", filename); exit (-1); }   /* modmap.c:196 */
  return rc;
}

/* ---- modutils -P: the painted file ---- */

/* modutils.c:260-273 ("-P"): plain FASTA / FASTQ text is parsed on the device and each batch painted there (mg_report.hip), its text
   written behind the next batch by the writer thread (mg_textout.c); gzip, a last line without its newline, FASTQ that breaks a rule: the host parser
   (from the first record the device parser has not handed on), each of its batches uploaded and painted the same way */
typedef struct { Modset *ms; MgTextOut *w; void *scratch; } PaintCtx;
static int paintDeviceBatch (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, void *stream)
{ PaintCtx *c = (PaintCtx *) v; (void) stream; return mgRefPaintBatchDevice (c->ms, dPacked, total, dOff, nReads, idBytes, idOff, c->w, &c->scratch); }
#define MG_PAINT_FILE_BATCH 128000000ull

int mgRefPaintFile (Modset *ms, const char *filename, FILE *out)
{
  char msg[600];
  if (!ms || !filename || !out) { mgSetErrorText ("mgRefPaintFile: invalid arguments"); return -1; }
  { FILE *f = fopen (filename, "r");
    if (!f) { snprintf (msg, sizeof (msg), "failed to open ref seq file %s", filename); mgSetErrorText (msg); return -1; }    /* modutils.c:262 */
    fclose (f);
  }
  if (mgIterRequireDevice ()) return -1;
  { MgSeqReader *r = mgSeqOpen (filename);                  /* (what the host parser cannot take -- and so the device parser neither: the reference's seqIOopenRead fails) */
    if (!r) { snprintf (msg, sizeof (msg), "failed to open ref seq file %s", filename); mgSetErrorText (msg); return -1; }
    mgSeqClose (r);
  }
  PaintCtx c; c.ms = ms; c.w = mgTextOutOpen (out); c.scratch = 0;
  U64 nSeq = 0, totLen = 0;
  int rc = mgSeqWalkFile (filename, paintDeviceBatch, 0, &c, MG_PAINT_FILE_BATCH, 1, &nSeq, &totLen);
  if (mgTextOutClose (c.w) && !rc) { mgSetErrorText ("mgRefPaintFile: write failed"); rc = -1; }
  mgRefPaintScratchFree (c.scratch);
  return rc ? -1 : 0;
}
