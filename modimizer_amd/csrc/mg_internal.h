/* mg_internal.h — private glue between mg_host.c (reference-compatible scalar API, plain C)
 * and mg_modsetdev.hip (device state).  Not part of the public ABI. */
#ifndef MG_INTERNAL_H
#define MG_INTERNAL_H
#include "modgpu.h"
#include "mg_knobs.h"
#include <stdlib.h>
#include <time.h>
#ifdef __cplusplus
extern "C" {
#endif
extern volatile int mgLiveDeviceModsets;          /* >0 when any Modset has a device table */
void mgHookDestroy (Modset *ms);                   /* modset is going away */
void mgHookHostRewrote (Modset *ms);               /* host arrays were rebuilt: drop the device table */
void mgHookNeedHost (Modset *ms, int wantIndex);   /* make value[] (and index[]) current; cheap when they are */
void mgHookNeedHostAll (Modset *ms, int wantIndex);/* also fold pending device depth counts into depth[] */
int  mgHookHasDevice (Modset *ms);
int  mgHookMergeDevice (Modset *ms1, Modset *ms2);   /* modsetMerge with ms1 on the device; 0 = done */
int  mgHookDeviceView (Modset *ms, const U64 **dValue1, const U16 **dDepth1, U32 *max);      /* entries 1 .. max on the device, counts folded; -1: no device table */
int  mgHookMergeDeviceArrays (Modset *ms1, const U64 *dValue2, const U16 *dDepth2, const U8 *dInfo2, U32 n2);   /* the second set as device arrays */
int  mgHookDeviceViewMake (Modset *ms, const U64 **dValue1, const U16 **dDepth1, U32 *max);  /* the same, the device table made from the host arrays if there is none */
int  mgHookPruneDevice (Modset *ms, int lo, int hi);  /* modsetDepthPrune on the device; 0 = done */
/* one GPU scan of one read for the iterator facade: *blk = malloc()ed replay block {U64 n; U64 kmer[n]; U32 posF[n]} */
int  mgIterScan (Seqhash *sh, const char *s, int len, U64 **blk);
int  mgIterRequireDevice (void);                   /* 0 when a HIP device is usable (cached); else the error is set */
void mgIterReleaseBuffers (void);                  /* the calling thread's iterator scratch (pinned buffers, stream) */
/* the same for the minimizer iterator: *rec = malloc()ed {U64 hash[n]; U32 posF[n]} */
int  mgIterMinScan (Seqhash *sh, const char *s, int len, U64 **rec, U64 *nOut);
/* the file front end on the device (mg_textgpu.hip; its windows, kernels and record ids: mg_textwin.hip, mg_textparse.hip, mg_textids.hip): plain FASTA / FASTQ text parsed by the GPU.  0 = done, -1 = error, -2 = not a
   file for this path (the host parser takes it), -3 = FASTQ text this parser leaves to the host parser from byte *resumeOff (a
   record start, line *resumeLine of the file; the counts are those of the records added so far) */
int  mgAddSequenceFileDevice (Modset *ms, const char *filename, U64 *nSeq, U64 *totLen, U64 *totHash, U64 *resumeOff, U64 *resumeLine);
/* the same for 10x reads (modutils.c:44): every batch through mgTrim10xDevice, records numbered from 1 through the file, before it is added */
int  mgAddSequenceFile10xDevice (Modset *ms, const char *filename, U64 *nSeq, U64 *totLen, U64 *totHash, U64 *resumeOff, U64 *resumeLine);
int  mgTextParseFileDevice (const char *filename, char **basesOut, int64_t **offsetsOut, int64_t *nSeqOut);   /* test hook: the parser's records as host arrays (malloc) */
/* the same parser for the callers that print record ids: every batch of complete records (device resident: packed bases, read
   offsets) with its ids (id r = idBytes + idOff[r], 0-terminated: seqio.c:303-304) to fn; a non-zero return of fn ends the file */
typedef int (*MgTextBatchFn) (void *ctx, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads, const char *idBytes, const U64 *idOff, void *stream);
int  mgTextForEachBatchDevice (const char *filename, MgTextBatchFn fn, void *ctx, U64 batchBases, U64 batchRecs, U64 *nSeq, U64 *totLen, U64 *resumeOff, U64 *resumeLine);   /* a batch is handed on (at a window's end) once it holds batchBases bases (0: the default, 1 Gbp) and batchRecs records, or the default's bases whatever the records */
/* the device halves of the modmap callers (mg_query.c, mg_reference.c): a batch that is already on the device */
int  mgQueryProcessDevice (MgReference *ref, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, int nReads, const char **names, FILE *out);
/* mgQueryFile's batches (mg_queryout.c): Push runs the device half now, a formatter and a writer thread put the lines out, in order, behind it */
typedef struct MgQueryPipe MgQueryPipe;
MgQueryPipe *mgQueryPipeOpen (MgReference *ref, FILE *out);
int  mgQueryPipePush (MgQueryPipe *p, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, int nReads, const char *idBytes, const U64 *idOff);
void mgQueryPipeClose (MgQueryPipe *p);                    /* returns when every line is written */
int  mgReferenceAddDevice (MgReference *ref, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, int nSeq, const char **names, bool isAdd);
void mgReferenceFinish (MgReference *ref, U64 totLen, bool isAdd, FILE *out);
void mgTextReleaseBuffers (void);
/* shared by the caller mirrors (mg_callers.c and the files split off it, the read set's files): not exported */
#define MG_HIDDEN __attribute__ ((visibility ("hidden")))
static inline void mgFatal (const char *what) { fprintf (stderr, "FATAL ERROR: %s: %s\n", what, mgLastError ()); exit (-1); }
static inline double mgMsBetween (const struct timespec *a, const struct timespec *b)      /* milliseconds from *a to *b */
{ return (b->tv_sec - a->tv_sec) * 1e3 + (b->tv_nsec - a->tv_nsec) * 1e-6; }
/* the ids of a device batch (id r = idBytes + idOff[r]) as the pointer array the callers take, into p[0 .. n) */
static inline void mgIdPointers (const char **p, const char *idBytes, const U64 *idOff, size_t n)
{ for (size_t i = 0 ; i < n ; ++i) p[i] = idBytes + idOff[i]; }
typedef struct { void *dPacked, *dOff; U64 total; U32 nReads; } MgDevBatch;     /* host bytes -> 2-bit words in HBM */
/* a file through the device text parser (devFn per batch: batchBases, batchRecs as mgTextForEachBatchDevice takes them), and where that one leaves it
   (-2, -3 above) through the host parser, from the start or from the record it stopped at: hostFn per batch, 0: every host batch is uploaded and handed
   to devFn with its ids.  Returns what the last leg returned */
MG_HIDDEN int mgSeqWalkFile (const char *filename, MgTextBatchFn devFn, int (*hostFn) (MgSeqBatch *, void *), void *ctx, U64 batchBases, U64 batchRecs, U64 *nSeq, U64 *totLen);
/* the host parser's batch loop (mg_seqio.c) for the file entry points (mg_seqfiles.c): every batch of the file through fn, the next one parsed while fn
   works on this one; from a record that starts at byte startOff of the text, line startLine, record startSeq + 1 (0 / 1 / 0: the whole file).  -1: no such
   file for this parser, else what fn returned last */
MG_HIDDEN int mgSeqForEachBatchFrom (const char *filename, size_t startOff, U64 startLine, U64 startSeq, int (*fn) (MgSeqBatch *, void *), void *ctx);
MG_HIDDEN void mgBatchUpload (MgDevBatch *b, const char *bases, const int64_t *offsets, int nReads);
MG_HIDDEN void mgBatchFree (MgDevBatch *b);
MG_HIDDEN FILE *mgTagOpen (const char *root, const char *tag, const char *mode);
/* The seed list of a device batch (mg_reads.hip): scan + lookups (insert: + inserts, modmap.c:109) with positions, in (read, pos) order, misses
   included.  The ONE place that guesses a capacity, makes the three arrays, and goes round again when the guess was short.
     arrays   device arrays of cap entries each (hipMalloc), grow-only: while cap covers what an attempt needs nothing is allocated, else all three
              are freed and made again with room for need + need * sparePct / 100 + 1 entries.  A caller that wants them for one call starts from a
              zeroed struct and ends with mgSeedBufsFree (or adopts the three pointers into its own scratch); one that keeps them between calls
              keeps the struct.  A failed allocation leaves "HIP error N (..) in <what>" and the struct zeroed.
     retry    the first attempt offers min (guess, totalBases + 1) entries.  If it ends in MG_ERR_CAPACITY with a count above what was offered, the
              arrays grow to exactly that count and the call runs once more: one retry, for lookups and inserts alike (the count is known before
              anything is inserted, so nothing is inserted twice).  Any other status, and a second MG_ERR_CAPACITY, comes back as it is with
              mgLastError () as the inner call left it -- a set that is full among them, whose count is not above the capacity; *nSeeds is set then, too.
     scanWith the hasher the batch is scanned with, 0: ms->hasher.  It has the set's k, or the call is MG_ERR_ARG.
     empty    totalBases == 0 or nReads == 0: *nSeeds = 0, nothing is allocated.  A set with max == 0: every index is 0, *nSeeds is the scan's count.
   The callers' kernels read the arrays below *nSeeds only. */
typedef struct { U32 *ix, *posF, *rid; U64 cap; int sparePct; } MgSeedBufs;
MG_HIDDEN MgStatus mgSeedsOfBatch (Modset *ms, const Seqhash *scanWith, int insert, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                   U64 guess, MgSeedBufs *bufs, U64 *nSeeds, void *stream);
MG_HIDDEN void mgSeedBufsFree (MgSeedBufs *bufs);
static inline U64 mgSeedGuess (int w, U64 totalBases)     /* modimizers are one k-mer in w: half as many again, and room for a short batch's noise */
{ U64 g = totalBases / (U64) (w > 0 ? w : 1); g += g / 2 + 65536; return g < totalBases + 1 ? g : totalBases + 1; }
/* queryProcess on the device (mg_chain.hip): per read the tallies of its "Q" line and its "M" blocks */
typedef struct { U32 nSeeds, missed, copy1, copy2, copyM, nM; } MgChainQ;
typedef struct { U32 pos0, posN, id0, off0, offN; int n1, n2; U32 span; } MgChainM;
MG_HIDDEN int  mgChainQueryDevice (const MgReference *ref, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                   MgChainQ *hQ, MgChainM **hMOut, U32 maxM, int hQPinned);
MG_HIDDEN void mgChainForget (const MgReference *ref);
#define MG_QUERY_MAXM 16                               /* "M" blocks of a read that the chain kernel keeps; a read with more takes the long way (mg_query.c) */
/* the "Q" / "M" lines of a batch whose tallies and blocks are on the host (mg_queryout.c): formatted by a team of threads and written to out, in order;
   *msFormat, *msWrite are added to.  Returns the team's size */
MG_HIDDEN int  mgQueryLinesOut (const MgReference *ref, const MgChainQ *q, const MgChainM *m, const int64_t *offsets, int nReads, const char **names, FILE *out,
                                double *msFormat, double *msWrite);
MG_HIDDEN int  mgQueryVerbose (void);                  /* modmap's -v (mgSetVerbose, mg_query.c): every batch takes the long way */
/* the Reference built on the device (mg_refpack.hip): a batch's seeds appended (modmap.c:110-117), then copy classes + referencePack (modmap.c:125-129,74-91) into the caller's arrays */
MG_HIDDEN MgStatus mgRefBuildAppend (MgReference *ref, const U32 *dIx, const U32 *dPosF, const U32 *dRid, U64 n, U32 idBase, U32 *appended);
MG_HIDDEN int mgRefPackedTallies (MgReference *ref, U32 tallies[3]);      /* 1: packed on the device, nothing added since */
MG_HIDDEN MgStatus mgRefBuildFinish (MgReference *ref, U32 *hIndex, U32 *hOffset, U32 *hId, U32 *hDepth, U32 *hRev, U32 *hLoc, U8 *hInfo, U32 tallies[3]);
MG_HIDDEN void *mgPinnedAlloc (size_t bytes);          /* page-locked host memory (0: none to be had) */
MG_HIDDEN void mgPinnedFree (void *p);
MG_HIDDEN MgStatus mgCopyOutPinned (void *dstPinned, const void *srcDev, size_t bytes, void *stream);   /* device -> page-locked block by a kernel (not the copy engine), waited for */
MG_HIDDEN void mgChainReleaseBuffers (void);
MG_HIDDEN void mgQueryReleaseBuffers (void);           /* the query path's cached buffers: page-locked blocks and line buffers (mg_queryout.c), device arrays (mg_chain.hip) */
MG_HIDDEN void mgChainScratchKeep (int on);      /* 1: the query's device arrays stay allocated between batches; 0: ends that (and frees them) */
/* a hit of a read: its mod, bit 31 set for forward orientation (modasm.c:22) */
#define MG_TOPBIT  0x80000000u
#define MG_TOPMASK 0x7fffffffu
/* a read set on the host as the device entry points below take it: the modset's info[msMax + 1] and depth[msMax + 1], hit[totHit], dx[totHit],
   hitStart[nReads + 2] and len[nReads + 1] (reads from 1; hitStart[nReads + 1] = totHit), invStart[msMax + 2], invSpace[invStart[msMax + 1]]; w: the hasher's;
   run: the reference's RUN for -T.  What a pass is about to write, or reads in a state that is not the set's yet, is a parameter of its own */
typedef struct { U32 msMax; int w, run; const U8 *info; const U16 *depth; const U32 *hit; const U16 *dx; U64 totHit; const U64 *hitStart; const int *len; U32 nReads;
                 const U64 *invStart; const U32 *invSpace; } MgRsView;
/* readsetFileRead's per-read loop on the device (mg_chain.hip): hit lists, distances, counts, hits per mod */
MG_HIDDEN int  mgReadsetSeedsDevice (Modset *ms, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                     U64 *hHitStart, U32 *hNMiss, U32 **dHitOut, unsigned short **dDxOut, U32 *dDepthAccum);
/* the per-mod side of the read set on the device (mg_rsdev.hip): hit counts kept across a file's batches; depth[], invStart[], invSpace[], nCopy[] at its end */
MG_HIDDEN MgStatus mgReadsetDevBegin (const void *rs, U32 msMax, U32 **dDepth);
MG_HIDDEN MgStatus mgReadsetFinishDevice (const void *rs, Modset *ms, const MgRsView *v, U16 *hDepth16, U64 *hInvStart, U32 **hInvSpace, int *hNCopy);
MG_HIDDEN void mgReadsetDevForget (const void *rs);
MG_HIDDEN void mgReadsetDevAppendHits (const void *rs, const U32 *dHit, U64 n);      /* a batch's hit list kept on the device for the end of the file */
/* modasm -C / -P over a read set on the host (mg_rsdev.hip): 0 = done, 1 = no room on the device (the caller's host loops take it), -1 = failed */
MG_HIDDEN int mgReadsetCleanDevice (const MgRsView *v, U8 *hInfo, int *hNCopy, U32 counts[3]);      /* hInfo: in and out */
MG_HIDDEN int mgReadsetPropertiesDevice (const MgRsView *v, int *hTally, U32 **hEv, U32 *nEv);
MG_HIDDEN int mgReadsetCopyTallyDevice (const MgRsView *v, const U8 *hInfo, int *hNCopy);      /* invBuild's nCopy[] from hInfo[], the info[] to be */
/* modasm's overlap passes (mg_overlap.hip): the pure record of findOverlaps (modasm.c:314-418) per (query, partner) with nHit >= 3.  nPlus / nMinus: as the
   "RH" line prints them (after the order test's decrements); flags: 1 isPlus, 2 isContained */
typedef struct { U32 iy; U16 nHit, nBadOrder, nBadFlip, nPlus, nMinus, flags; } MgOvlRec;
typedef struct MgOvlDev MgOvlDev;
/* Open: the set's arrays go to the device once per call; 0 = done, 1 = the device has no room (the
   caller's host loops take the call), -1 = failed.  Batch: queries[0 .. nq) (read numbers, checked by the caller; their hits together and their candidates
   together below 2^31): nRepeat[nq], start[nq + 1], *recs (malloc ()ed: start[nq] records, a query's by nHit descending then arrival); diag[1..3] are added to.
   0 / 1 (no room for this batch) / -1 */
MG_HIDDEN int  mgOvlDevOpen (MgOvlDev **d, const MgRsView *v);
MG_HIDDEN int  mgOvlDevBatch (MgOvlDev *d, const U32 *queries, U32 nq, U32 *nRepeat, U64 *start, MgOvlRec **recs, U64 diag[4]);
MG_HIDDEN void mgOvlDevClose (MgOvlDev *d);
MG_HIDDEN U64  mgOvlDevCandBudget (void);      /* candidates per batch that the free device memory allows */
/* modasm -R / -T (mg_rdna.hip; the host loops are mg_rs_rdna.c's).  checkMod (modasm.c:564-568) and the rules of testMods per (tested mod i, partner m)
   (modasm.c:658-705) are written once, here, for the kernels and the host loops alike */
#ifdef __HIPCC__
#define MG_BOTH __host__ __device__
#else
#define MG_BOTH
#endif
static inline MG_BOTH int mgRdnaCheckMod (unsigned info) { return (info & 3u) != 0 && (info & (MS_REPEAT | MS_RDNA)) == MS_RDNA; }
enum { MG_LD_MOD2 = 1, MG_LD_GOOD = 2, MG_LD_SPLIT = 4, MG_LD_BAD_M = 8, MG_LD_BAD_I = 16, MG_LD_PLUS = 32 };
typedef struct { U32 m; int flags, n, vmin, xmin, vmax, xmax; } MgLdCell;      /* a "ZZ-TEST" line less i and the depths; flags: what the pair adds where */
/* n occurrences of m around i with signed distances dmin .. dmax; start[0 .. nStart), end[0 .. nEnd): the suffix-summed counts (modasm.c:651-654) of i;
   run: the reference's RUN.  0, or -1 where the reference asserts or reads a cell beyond an array's extent */
static inline MG_BOTH int mgRdnaLdRule (int n, int dmin, int dmax, const int *start, int nStart, const int *end, int nEnd, int depthM, int run, MgLdCell *c)
{
  int f = 0;
  if (dmin > 0)
    { const int xmin = dmin, xmax = dmax;
      if (xmin >= nEnd || xmax >= nEnd) return -1;
      const int e = end[xmin];
      if (n < depthM && n * 2 < e) { f |= MG_LD_MOD2; if (run > 3) f |= MG_LD_BAD_M; }
      if (n == depthM || n >= 0.8 * e) f |= MG_LD_GOOD;
      if (n == 1 && e >= 10) f |= MG_LD_BAD_I;                      /* modasm.c:673: i's own entry */
      c->flags = f | MG_LD_PLUS; c->n = n; c->vmin = e; c->xmin = xmin; c->vmax = end[xmax]; c->xmax = xmax;
    }
  else
    { const int xmax = -dmin; int xmin = -dmax;
      if (xmin < 0) { f |= MG_LD_SPLIT; xmin = xmax; }
      if (xmin >= nStart || xmax >= nStart) return -1;
      const int s = start[xmin];
      if (n < depthM && n * 2 < s) { f |= MG_LD_MOD2; if (run > 3) f |= MG_LD_BAD_M; }
      else if (n == 1 && s >= 10) f |= MG_LD_BAD_M;                 /* modasm.c:695: m's entry */
      if (n == depthM || n >= 0.8 * s) f |= MG_LD_GOOD;
      c->flags = f; c->n = n; c->vmin = s; c->xmin = xmin; c->vmax = start[xmax]; c->xmax = xmax;
    }
  return 0;
}
/* The reference makes its two count arrays with arrayReCreate (.., 20000, int) per tested mod (modasm.c:619-620), which clears the first 20000 cells of an
   array that is already there (array.c:103): from the second tested mod whose array passes that extent on it counts on top of stale, suffix-summed cells.
   That is where it breaks (its own assert at modasm.c:649-650 fires once the sums overflow); the call is refused there, by device and host loops alike */
#define MG_RDNA_CLEARED 20000
/* per read 1 .. nReads the hit number of the 200th hit on a mod with qual[] set, from the front (n200, 0: fewer) and, if there is one, from the back
   without ever looking at hit 0 (m200): modasm.c:781-802.  0 / 1 (no room on the device) / -1 */
MG_HIDDEN int mgRdnaN200Device (const MgRsView *v, const U8 *hQual, int *hN200, int *hM200);
/* testMods over a set on the host.  tested[nTested] ascending, partner[nPartner] ascending (every tested mod is a partner).  Out: per tested mod
   { nGood, nMod2, nSplit } in res3, badLD[msMax + 1] and splitLD[msMax + 1] added to (zeroed by the caller); wantCells: *cells (malloc ()ed) holds
   cellStart[nTested] records, those of tested mod t at [cellStart[t], cellStart[t + 1]), m ascending.  batch: tested mods per batch, 0: by the device's
   free memory.  diag[0] batches, [3] partner occurrences.  grid[4]: the partner tiles, the least and the greatest share of the visits over the batches, the cells per count array.  0 / 1 (no room) / -1; -2: a visit or a cell the reference cannot do (*badMod: the tested mod); -3: a second tested mod whose count array passes
   MG_RDNA_CLEARED cells */
MG_HIDDEN int mgRdnaTestModsDevice (const MgRsView *S, const U32 *tested, U32 nTested, const U32 *partner, U32 nPartner, U32 batch, int wantCells,
                                    int *res3, int *badLD, int *splitLD, U64 *cellStart, MgLdCell **cells, U64 diag[4], U32 grid[4], U32 *badMod);
MG_HIDDEN MgStatus mgModsetAdoptDepthDevice (Modset *ms, const U16 *dDepth16);      /* the device table's depth copy = dDepth16[0 .. max] (mg_modsetdev.hip) */
/* modutils' reports (mg_report.hip): text formatted on the device, copied out and written in order by a writer thread (mg_textout.c) */
typedef struct MgTextOut MgTextOut;
MG_HIDDEN MgTextOut *mgTextOutOpen (FILE *out);
MG_HIDDEN int  mgTextOutFromDevice (MgTextOut *w, const void *dSrc, size_t bytes);   /* copied into page-locked blocks now, written behind the caller, in order */
MG_HIDDEN int  mgTextOutClose (MgTextOut *w);                /* returns when every byte is written; -1 if a write failed */
MG_HIDDEN int  mgRefPaintBatchDevice (Modset *ms, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                      const char *idBytes, const U64 *idOff, MgTextOut *w, void **scratch);   /* modutils.c:262-270 over a device batch; 0 / -1 */
MG_HIDDEN void mgRefPaintScratchFree (void *scratch);
MG_HIDDEN void mgSetErrorText (const char *msg);
/* the file mover of the device text parser (mg_textwin.hip), for the other reader of plain text (mg_settext.hip) */
MG_HIDDEN int mgTextReadParallel (int fd, unsigned char *dst, size_t n, int64_t off);      /* [off, off + n) of the file into dst by the parser's team of threads; 0 = read */
MG_HIDDEN size_t mgTextWindowBytes (size_t fileSize);      /* text per window: MODGPU_TEXT_WINDOW_KB, or the parser's default for a file of that size; whole tiles of 4 KiB */
/* The parser's window loop for another consumer of FASTA / FASTQ text (mg_composition.hip): the text -- whatever `fill` produces: a plain
   file by the parser's team of threads, an inflated stream, a block of host memory -- goes through the parser's own page-locked and device
   window buffers, two of each, and `fn` launches its kernels on `stream` for every window in order while the next one is read and crosses
   the link.  fill (src, dst, cap, off): up to cap bytes that follow byte off of the text into dst; the count, less than cap only at the
   text's end, (size_t) -1 on a read error.  fn: 0, or non-zero to end the walk (the streamer then returns -1, the error is fn's).
   sizeHint: the text's size where it is known (the window is the parser's for a file of that size; MODGPU_TEXT_WINDOW_KB comes first).
   Returns 0 with every kernel of every window finished; *nWindows is set either way */
typedef struct { const unsigned char *dText, *hText; size_t n; U64 off; U32 prevByte; U64 index; U32 first, last; } MgTextWindow;      /* prevByte: the byte before the window, '\n' before the text's first; first, last: the window's own first and last byte; hText: the window in page-locked host memory, 0 from a device source */
typedef size_t (*MgTextFillFn) (void *src, unsigned char *dst, size_t cap, U64 off);
typedef int (*MgTextWindowFn) (void *ctx, const MgTextWindow *w, void *stream);
MG_HIDDEN int mgTextStreamWindows (size_t sizeHint, MgTextFillFn fill, void *src, MgTextWindowFn fn, void *ctx, U64 *nWindows);
/* The same loop over a source that fills the window's DEVICE buffer (blocked gzip inflated on the device, mg_bgzfsrc.hip): no page-locked copy of the
   window exists, the consumers read w->first and w->last.  dfill (src, dDst, cap, off, stream, &n, &more, &first, &last): up to cap bytes that follow byte
   off into dDst by work on `stream` that is over when it returns; n may be short of cap anywhere, *more says whether text follows; 0, or -1 with the error set */
typedef int (*MgTextDevFillFn) (void *src, unsigned char *dDst, size_t cap, U64 off, void *stream, size_t *n, int *more, U32 *first, U32 *last);
MG_HIDDEN int mgTextStreamWindowsDev (size_t sizeHint, MgTextDevFillFn dfill, void *src, MgTextWindowFn fn, void *ctx, U64 *nWindows);
/* mg_inflate.hip for mg_bgzfsrc.hip: mgInflateMembersDevice with the caller's device scratch (mgInflateWorkBytes (n)), adding to the thread's mgInflateDiag */
MG_HIDDEN MgStatus mgInflateRun (const U8 *dComp, U64 compBytes, const MgGzMember *members, U32 n, U8 *dOut, U64 outBytes, void *dWork, U32 *status, U32 *nBad, void *stream);
MG_HIDDEN size_t mgInflateWorkBytes (U32 n);
MG_HIDDEN void mgInflateDiagReset (void);
MG_HIDDEN void mgInflateDiagUploaded (U64 bytes);
/* A file that is blocked gzip from its first byte to its last as a source of text on the device (mg_bgzfsrc.hip).  Open: 0 and *out, -2 = not such a
   file (no error is set: the caller reads it as any gzip), -1 = error.  fd stays the caller's.  Fill: the MgTextDevFillFn contract, below `limit` */
typedef struct MgBgzfSrc MgBgzfSrc;
MG_HIDDEN int mgBgzfSrcOpen (const char *name, int fd, U64 fileSize, MgBgzfSrc **out);
MG_HIDDEN void mgBgzfSrcClose (MgBgzfSrc *s);
MG_HIDDEN void mgBgzfSrcRewind (MgBgzfSrc *s);
MG_HIDDEN U64 mgBgzfSrcTextBytes (const MgBgzfSrc *s);
MG_HIDDEN int mgTextFirstByte (const char *filename);      /* the first byte of the file's text, through blocked or ordinary gzip if that is what the file starts with; -1: none */
MG_HIDDEN void mgBgzfSrcOneWalk (MgBgzfSrc *s);      /* before the first fill: the file is walked once, so its compressed bytes do not stay on the device (no Rewind after it) */
/* the text's first byte and its last min (cap, text) bytes, from the first and the last non-empty members inflated on the host; 0, -2 = one of them does not inflate */
MG_HIDDEN int mgBgzfSrcEdges (MgBgzfSrc *s, unsigned char *first, unsigned char *tail, size_t cap, size_t *tailN);
MG_HIDDEN int mgBgzfSrcFill (MgBgzfSrc *s, unsigned char *dDst, size_t cap, U64 off, U64 limit, void *stream, size_t *n, int *more, U32 *first, U32 *last);
/* mg_gunzip.hip: an ordinary gzip stream whose compressed bytes dComp[0 .. n) are on the device, inflated batch by batch (mg_gunzip_core.h); fd: the same
   file, for the headers and trailers the host looks at.  Next: the stream's next text (*dText, *n bytes, the stream's until the next call) by work on
   `stream` that is over when it returns, adding to the thread's mgGunzipDiag; 0, or -1 with the error set (*status and *errOff: a wrong stream) */
typedef struct MgGunzipDev MgGunzipDev;
MG_HIDDEN int mgGunzipDevOpen (const U8 *dComp, U64 n, int fd, U32 chunkBytes, U32 batchChunks, U32 symbolsPerChunk, MgGunzipDev **out);
MG_HIDDEN void mgGunzipDevClose (MgGunzipDev *g);
MG_HIDDEN void mgGunzipDevRewind (MgGunzipDev *g);
MG_HIDDEN int mgGunzipDevNext (MgGunzipDev *g, void *stream, const U8 **dText, size_t *n, int *done, U32 *status, U64 *errOff);
/* One walk: the stream's compressed bytes are not all on the device (Open with dComp 0, then this before the first Next).  Before it runs a batch the
   stream says which file bytes [from, to) the batch reads; fn has them on the device by work on `stream` and returns *comp with *comp + o the file's
   byte o for the offsets o it holds from `from` on, and *end >= to where they end.  A decode that runs out of bytes below the file's end ends the
   batch's chain there, or makes the stream ask again for twice as much if it was the batch's first chunk.  fn: 0, -1 with the error set */
typedef int (*MgGunzipRangeFn) (void *ctx, U64 from, U64 to, void *stream, const U8 **comp, U64 *end);
MG_HIDDEN void mgGunzipDevRange (MgGunzipDev *g, MgGunzipRangeFn fn, void *ctx);
MG_HIDDEN void mgGunzipDiagReset (void);
/* An ordinary gzip file as a source of text on the device (mg_gzipsrc.hip), with the contract of MgBgzfSrc.  Open: -2 = not a file for this path (not
   gzip, a 'BC' first member, smaller than MODGPU_GZIP_MIN_KB, MODGPU_GZIP_HOST=1 -- MG_GZIP_ANY: the last two are not asked -- or more than the device
   holds).  MG_GZIP_ONE_WALK: the caller walks the text once, so the compressed file passes through a bounded range on the device and does not stay
   (mgGzipSrcDiag); a file of any size is taken, and Rewind is an error (-1) */
typedef struct MgGzipSrc MgGzipSrc;
#define MG_GZIP_ANY 1
#define MG_GZIP_ONE_WALK 2
MG_HIDDEN int mgGzipSrcOpen (const char *name, int fd, U64 fileSize, int flags, MgGzipSrc **out);
MG_HIDDEN void mgGzipSrcClose (MgGzipSrc *s);
MG_HIDDEN int mgGzipSrcRewind (MgGzipSrc *s);
MG_HIDDEN int mgGzipFirstByte (const unsigned char *head, size_t n);      /* the first byte of the text of the gzip file that begins head[0 .. n), by zlib on the host; -1: the head does not hold it */
MG_HIDDEN int mgGzipSrcFirstByte (const MgGzipSrc *s);      /* the text's first byte, from the file's head inflated on the host; -1: the head does not say */
MG_HIDDEN U64 mgGzipSrcSizeHint (const MgGzipSrc *s);
MG_HIDDEN int mgGzipSrcFill (MgGzipSrc *s, unsigned char *dDst, size_t cap, U64 off, U64 limit, void *stream, size_t *n, int *more, U32 *first, U32 *last);
/* mg_deflate.hip for mg_bgzfsink.hip: mgDeflateBlocksDevice on `stream` with device scratch that outlives the call (it only grows; Free drops it),
   adding to the thread's mgDeflateDiag */
typedef struct MgDeflateWork MgDeflateWork;
MG_HIDDEN MgDeflateWork *mgDeflateWorkNew (void);
MG_HIDDEN void mgDeflateWorkFree (MgDeflateWork *w);
MG_HIDDEN MgStatus mgDeflateRun (MgDeflateWork *w, const U8 *dText, U64 textBytes, const MgGzBlock *blocks, U32 n, U8 *dOut, U64 outBytes, U64 *memberOff, void *stream);
MG_HIDDEN void mgDeflateDiagReset (void);
/* Text on the device as a blocked-gzip (BGZF) file (mg_bgzfsink.hip): what is appended is cut into blocks of MODGPU_BGZF_BLOCK bytes wherever the appends
   end, whole blocks are deflated on the device (mg_deflate.hip) and their packed members handed to `emit` in file order -- a device range, or for the
   end-of-file member host bytes -- of at most mgBgzfSinkEmitMax () bytes a call, and is done with them when it returns; the tail of less than a block stays on the device.  Close (flush = 1)
   deflates the tail and emits the end-of-file member.  Every call: 0, or -1 with the error set (emit's own, if it was emit that failed) */
typedef struct MgBgzfSink MgBgzfSink;
typedef int (*MgBgzfEmitFn) (void *ctx, const unsigned char *src, size_t n, int onDevice, void *stream);
MG_HIDDEN MgBgzfSink *mgBgzfSinkOpen (MgBgzfEmitFn emit, void *ctx, const char *what, U64 textHint);      /* textHint: about how much text will come: a short text gets a short row; 0 = no idea */
MG_HIDDEN size_t mgBgzfSinkEmitMax (const MgBgzfSink *s);
MG_HIDDEN int mgBgzfSinkAppendDevice (MgBgzfSink *s, const unsigned char *dSrc, size_t n);      /* (the bytes are there: their producer has been waited for) */
MG_HIDDEN int mgBgzfSinkAppendRun (MgBgzfSink *s, int byte, U64 n);
MG_HIDDEN int mgBgzfSinkAppendHost (MgBgzfSink *s, const void *p, size_t n);
MG_HIDDEN int mgBgzfSinkClose (MgBgzfSink *s, int flush);
/* K1 of the FASTA parser for that consumer: tileEvent[t] = the code (txEvent below) of the last event of tile t of the window, 0: none */
MG_HIDDEN int mgTextLaunchEventTiles (const unsigned char *dText, size_t n, U64 textBase, U32 prevByte, U64 *dTileEvent, void *stream);
#ifdef __HIPCC__
/* the per-byte rules of the device text parser, for its kernels and those of the other consumer.  Both cut a window into tiles of
   MG_TEXT_TILE bytes, one workgroup of 256 threads with one 16-byte load each (the files name their own thread count: tests/test_abi.py
   resolves the workgroup primitives' THREADS through the file that calls them) */
#define MG_TEXT_TILE 4096
/* a thread's 16 bytes and the byte before them */
static __device__ __forceinline__ void txLoad (const unsigned char *text, U64 n, U64 at, U32 prevByte, unsigned char *b, U32 *prev)
{
  uint4 v = make_uint4 (0, 0, 0, 0);
  if (at + 16 <= n) v = *reinterpret_cast<const uint4 *> (text + at);
  else { unsigned char t[16]; for (int j = 0 ; j < 16 ; ++j) t[j] = at + j < n ? text[at + j] : 0; __builtin_memcpy (&v, t, 16); }
  __builtin_memcpy (b, &v, 16);
  *prev = at ? text[at - 1] : prevByte;
}
/* the event code of byte i of the window (0: no event): newline -> even, record start -> odd; a later event has a larger code */
static __device__ __forceinline__ U64 txEvent (U32 c, U32 prev, U64 filePos)
{
  if (c == '\n') return (filePos + 1) << 1;
  if (c == '>' && prev == '\n') return ((filePos + 1) << 1) | 1;
  return 0;
}
/* the code of the last event among a thread's bytes, 0: none (prev: the byte before them; base: the text offset of b[0]) */
static __device__ __forceinline__ U64 txLastEvent (const unsigned char *b, U64 at, U64 n, U32 prev, U64 base)
{
  U64 last = 0;
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j) { if (at + j < n) { const U64 e = txEvent (b[j], prev, base + j); if (e) last = e; } prev = b[j]; }
  return last;
}
/* the newlines among a thread's bytes (FASTQ: the line a byte belongs to is the number of newlines before it) */
static __device__ __forceinline__ U32 txNewlines (const unsigned char *b, U64 at, U64 n)
{
  U32 c = 0;
#pragma unroll
  for (int j = 0 ; j < 16 ; ++j) c += (at + j < n && b[j] == '\n') ? 1u : 0u;
  return c;
}
#endif
/* modutils -rt (mg_settext.hip): the `want` lines that follow byte bodyOff of the file parsed on the device against the strict grammar
   (modgpu.h), tokens of k bytes; 0 = all of them passed, the three device arrays (hipMalloc: mgDeviceFree) hold them; 1 = some line
   does not pass, or there are fewer (nothing is returned); -1 = error */
MG_HIDDEN int mgSetTextParseDevice (const char *filename, U64 bodyOff, U64 want, int k, U64 **dKey, U16 **dDepth, U8 **dInfo);
/* the lines' values into the (fresh) set: inserted in order, every k-mer's last line gives its depth and info; ms->max, depth[], info[]
   current on return.  0 / -1.  ...HostArrays: the same from host arrays (the lines the host parsed) */
MG_HIDDEN int mgSetTextFillDevice (Modset *ms, const U64 *dKey, const U16 *dDepth, const U8 *dInfo, U64 n);
MG_HIDDEN int mgSetTextFillHostArrays (Modset *ms, const U64 *key, const U16 *depth, const U8 *info, U64 n);
/* mg_modutils.hip.  The census behind mgAdd10xDiag, kept per thread: a new file, a batch that went through the trim, a leg of the host parser */
MG_HIDDEN void mgAdd10xDiagReset (void);
MG_HIDDEN void mgAdd10xDiagBatch (U32 nReads, U64 firstOrdinal, U64 dropped);
MG_HIDDEN void mgAdd10xDiagHostLeg (void);
/* the summary's counters of a set with a device table: [0 .. 65536) entries by depth (pending counts included), [65536 .. 65540) by
   info & 3; ms->max is brought up to date.  0 / 1 (the set has no device table) / -1 */
MG_HIDDEN int mgSummaryCountersDevice (Modset *ms, U64 *counters);
/* element count of the reference's Array after appending elements 0..n-1 (array.c:144-170,180-183) */
MG_HIDDEN int mgRefArrayDim (int first, int size, int n);
#ifdef __cplusplus
}
#endif
#endif
