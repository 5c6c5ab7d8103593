/* mg_callers.c — C counterparts of the reference's hot-path callers for sequences already in memory: upload a batch, call the
 * device half.
 *   modutils: addSequenceFile's loop + report (modutils.c:33-51), -P on records in memory (modutils.c:260-273)
 *   modmap  : Reference build (modmap.c:49-134) and queryProcess (modmap.c:188-281)
 * The device halves and what stays on the host around them: mg_reference.c, mg_query.c + mg_queryout.c, mg_textout.c; the file
 * entry points: mg_seqfiles.c; a set as text: mg_modsettext.c; the .mod + .ref files: mg_reffiles.c.
 */
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"
#include "mg_internal.h"

/* ---- packed batch on the device (host bytes -> 2-bit words -> HBM) ---- */

void mgBatchUpload (MgDevBatch *b, const char *bases, const int64_t *offsets, int nReads)
{
  b->nReads = (U32) nReads;
  b->total = nReads ? (U64) offsets[nReads] : 0;
  size_t nw = mgPackedWords (b->total);
  if (mgDeviceAlloc (&b->dPacked, nw * 4) || mgDeviceAlloc (&b->dOff, ((size_t) nReads + 1) * 8)) mgFatal ("device alloc");
  if (mgUploadPack (bases, b->total, (U32 *) b->dPacked, 0) || mgMemcpyH2D (b->dOff, offsets, ((size_t) nReads + 1) * 8, 0)
      || mgStreamSynchronize (0)) mgFatal ("H2D");
}

void mgBatchFree (MgDevBatch *b) { mgDeviceFree (b->dPacked); mgDeviceFree (b->dOff); }

/* ---------------------------------- modutils ---------------------------------- */

int mgAddSequences (Modset *ms, const char *bases, const int64_t *readOffsets, int nReads, FILE *out)
{
  int64_t nHash = mgAddSequenceBatch (ms, bases, readOffsets, nReads);
  if (nHash < 0) return -1;
  U64 totLen = nReads ? (U64) readOffsets[nReads] : 0;
  fprintf (out, "added %llu sequences total length %llu total hashes %llu, new max %u\n",
           (unsigned long long) nReads, (unsigned long long) totLen, (unsigned long long) nHash, ms->max);
  return 0;
}

/* modutils.c:260-273 on records already in memory: one batch, the names packed into one block as the device parser hands them on */
int mgRefPaint (Modset *ms, const char *bases, const int64_t *offsets, int nSeq, const char **names, FILE *out)
{
  if (!ms || !out || nSeq < 0 || (nSeq && (!bases || !offsets || !names))) { mgSetErrorText ("mgRefPaint: invalid arguments"); return -1; }
  if (mgIterRequireDevice ()) return -1;
  if (!nSeq) return 0;
  U64 *idOff = (U64 *) malloc ((size_t) nSeq * 8); size_t tot = 0;
  if (!idOff) mgFatal ("out of memory");
  for (int r = 0 ; r < nSeq ; ++r) { idOff[r] = tot; tot += strlen (names[r] ? names[r] : "") + 1; }
  char *ids = (char *) malloc (tot);
  if (!ids) mgFatal ("out of memory");
  for (int r = 0 ; r < nSeq ; ++r) { const char *s = names[r] ? names[r] : ""; memcpy (ids + idOff[r], s, strlen (s) + 1); }
  MgDevBatch b; mgBatchUpload (&b, bases, offsets, nSeq);
  MgTextOut *w = mgTextOutOpen (out);
  void *scratch = 0;
  int rc = mgRefPaintBatchDevice (ms, (const U32 *) b.dPacked, b.total, (const U64 *) b.dOff, (U32) nSeq, ids, idOff, w, &scratch);
  if (mgTextOutClose (w) && !rc) { mgSetErrorText ("mgRefPaint: write failed"); rc = -1; }
  mgRefPaintScratchFree (scratch);
  mgBatchFree (&b);
  free (ids); free (idOff);
  return rc;
}

/* ---------------------------------- modmap ---------------------------------- */

int mgReferenceRead (MgReference *ref, const char *bases, const int64_t *offsets, int nSeq,
                     const char **names, bool isAdd, FILE *out)
{
  const int timing = mgKnobs ()->seedTiming == 1;          /* dev */
  struct timespec c0, c1, c2, c3; clock_gettime (CLOCK_MONOTONIC, &c0);
  MgDevBatch b; mgBatchUpload (&b, bases, offsets, nSeq);
  clock_gettime (CLOCK_MONOTONIC, &c1);
  mgReferenceAddDevice (ref, (const U32 *) b.dPacked, b.total, (const U64 *) b.dOff, nSeq, names, isAdd);
  mgBatchFree (&b);
  clock_gettime (CLOCK_MONOTONIC, &c2);
  mgReferenceFinish (ref, nSeq ? (U64) offsets[nSeq] : 0, isAdd, out);
  clock_gettime (CLOCK_MONOTONIC, &c3);
  if (timing) fprintf (stderr, "mgReferenceRead: pack + upload %.1f ms, scan + insert + append %.1f ms, finish (mirror, classes, pack) %.1f ms\n",
                       mgMsBetween (&c0, &c1), mgMsBetween (&c1, &c2), mgMsBetween (&c2, &c3));
  return 0;
}

int mgQueryProcess (MgReference *ref, const char *bases, const int64_t *offsets, int nReads,
                    const char **names, FILE *out)
{
  if (nReads <= 0) return 0;
  MgDevBatch b; mgBatchUpload (&b, bases, offsets, nReads);
  int rc = mgQueryProcessDevice (ref, (const U32 *) b.dPacked, b.total, (const U64 *) b.dOff, nReads, names, out);
  mgBatchFree (&b);
  return rc;
}
