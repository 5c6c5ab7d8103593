/* include/modgpu.h — C ABI of libmodgpu.so: modimizer's seqhash + modset hot path on MI355X (gfx950).
 *
 * Two layers, both plain C (pointers and sizes only, no C++/torch types):
 *
 *  (1) the reference's own seqhash.h / modset.h API with identical signatures and struct layouts,
 *      so modmap/modutils-style callers link against this library unchanged
 *      (reference seqhash.h:36-60, modset.h:30-69; struct layouts seqhash.h:15-34, modset.h:17-28).
 *      A caller built inside the reference tree keeps including the reference's own modset.h (its
 *      unmodified modutils.c / modmap.c link against libmodgpu.so as they are: oracle/Makefile builds
 *      them that way and tests/test_dropin.py runs them); a caller without the reference tree gets
 *      the same declarations, header-inline helpers included, from modgpu_compat.h.
 *
 *  (2) this file: batch entry points that carry the GPU path: whole batches of reads are scanned, the
 *      modimizers compacted in (read,pos) order, and inserted into / looked up in a device-resident
 *      modset table.  These replace the per-read loops of the reference callers
 *      (modutils.c:19-31, modmap.c:106-118, modmap.c:197-206).
 *
 * Using (2) next to the reference's headers: include the reference's modset.h FIRST, then this file.
 * It notices (MS_MINOR is a macro of modset.h:49; or define MODGPU_WITH_REFERENCE_HEADERS) and takes
 * Seqhash / Modset / U8..U64 from there instead of declaring them again.
 *
 * Error behaviour follows the reference: invalid parameters and capacity overflow print
 * "FATAL ERROR: ..." and exit(-1) (utils.c:19-30) in layer (1); layer (2) functions return a
 * non-zero MgStatus and leave a message retrievable with mgLastError().  There is no CPU fallback:
 * every batch entry point fails with MG_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef MODGPU_H
#define MODGPU_H

#include <stdio.h>
#include <stdint.h>
#include <stdbool.h>
#include <stddef.h>

#if defined (MODGPU_WITH_REFERENCE_HEADERS) || defined (MS_MINOR)
/* layer 1 comes from the reference's modset.h + seqhash.h + utils.h, already included */
#ifdef __cplusplus
extern "C" {
#endif
void mgSeqhashDestroy (Seqhash *sh) ;                       /* real symbols for the reference's header-inline destroys */
void mgSeqhashRCiteratorDestroy (SeqhashRCiterator *si) ;
#ifdef __cplusplus
}
#endif
#else
#include "modgpu_compat.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Layer 2: batch / device entry points (the GPU hot path).
 * ------------------------------------------------------------------------------------------ */

typedef enum {
  MG_OK = 0,
  MG_ERR_NO_DEVICE = 1,     /* no usable HIP device / runtime: there is no CPU fallback */
  MG_ERR_HIP = 2,           /* a HIP call failed; see mgLastError() */
  MG_ERR_ARG = 3,           /* invalid argument */
  MG_ERR_CAPACITY = 4,      /* output or modset capacity exceeded */
  MG_ERR_NOMEM = 5
} MgStatus ;

const char *mgLastError (void) ;
int  mgDeviceCount (void) ;                 /* 0 when no device; never initialises a context */
MgStatus mgSetDevice (int device) ;         /* device used by subsequent calls of this thread */
const char *mgVersion (void) ;                 /* "modgpu <version> (gfx950) src=<hash>" */
const char *mgSourceHash (void) ;             /* 16 hex digits: hash of the sources this binary was compiled from (csrc/mg_version.c) */

/* The per-read facade's latency switch (seqhash.c:154-196 behind modRCiterator).  A synchronous per-read call cannot
 * hide a kernel launch (13-15 us launch + poll whatever the length), so modRCiterator scans reads shorter than
 * MODGPU_ITER_HOST_BELOW bases (default: the measured crossover, 12288, or 8192 where w < 16; 0 = every read through the kernel) with the library's own scalar loop and
 * longer ones with one kernel launch; both write the same replay block.  mgIterScanHost is that scalar loop by itself
 * (tests pin it to the golden vectors, the oracle and the compiled reference without a GPU): the malloc()ed block
 * {U64 n; U64 kmer[n]; U32 pos | isF << 31 [n]} of one read.  It is not a fallback: modRCiterator die()s without a HIP
 * device whatever the read's length, and no batch entry point ever takes it. */
U64 *mgIterScanHost (const Seqhash *sh, const char *s, int len) ;
void mgReloadKnobs (void) ;                 /* the library reads its MODGPU_* environment knobs once; this reads them again (tests that set one between calls; not while another thread is inside the library) */
int  mgIterHostBelow (int below) ;          /* sets the crossover in bases (below < 0: only asks; 1 << 30: back to the defaults by w); returns the one in force before */

/* Device memory helpers so a host language needs no other HIP binding. */
MgStatus mgDeviceAlloc (void **dptr, size_t bytes) ;
MgStatus mgDeviceFree (void *dptr) ;
MgStatus mgMemcpyH2D (void *dst, const void *src, size_t bytes, void *stream) ;
MgStatus mgMemcpyD2H (void *dst, const void *src, size_t bytes, void *stream) ;
MgStatus mgMemsetD (void *dst, int byte, size_t bytes, void *stream) ;
MgStatus mgStreamSynchronize (void *stream) ;
/* Whole arrays between the device and PAGEABLE host memory at the link's speed: a team of host threads (mgXferThreadCount) moves the
 * array in 4 MiB pieces through page-locked blocks, one copy stream each (what modsetSyncToHost and mgReferenceRead mirror their
 * results with; a plain copy into pageable memory goes through the runtime's staging at a few GB/s).  Both wait for the device to be
 * idle first and return when the bytes are in place. */
MgStatus mgCopyD2HBig (void *hostDst, const void *devSrc, size_t bytes) ;
MgStatus mgCopyH2DBig (void *devDst, const void *hostSrc, size_t bytes) ;

/* 2-bit packed read layout in HBM: base i of the concatenated batch lives in bits
 * [30-2*(i%16), 32-2*(i%16)) of 32-bit word i/16 (first base in the most significant bits, so a
 * k-mer read left to right is a contiguous big-endian bit field).  Buffers are
 * mgPackedWords(n) words long: ceil(n/16) plus MG_PACK_PAD zero words of read-ahead slack.
 * Input bytes are bases 0..3 (seqio.c:643-652 after the N->0 patch of modmap.c:97); only the low
 * two bits of each byte are used. */
#define MG_PACK_PAD 8
size_t   mgPackedWords (U64 nBases) ;
void     mgPackHost (const char *bases, U64 nBases, U32 *words) ;
MgStatus mgPackDevice (const U8 *dBases, U64 nBases, U32 *dWords, void *stream) ;
MgStatus mgUnpackDevice (const U32 *dWords, U64 nBases, U8 *dBases, void *stream) ;
/* host bytes -> packed words in HBM (dPacked: mgPackedWords(n) words): PCIe copy in pieces + K1 on the device */
MgStatus mgUploadPack (const char *bases, U64 nBases, U32 *dPacked, void *stream) ;

/* Scan (seqhash.c:154-196 over a whole batch).
 * dPacked: the batch, reads concatenated without padding; dReadOffsets[nReads+1]: start of each
 * read in bases (offsets[0] = 0, offsets[nReads] = totalBases).
 * Outputs, in (read, pos) order, one entry per modimizer:
 *   dKmer[i]  canonical k-mer (seqhash.c:183)
 *   dPosF[i]  pos within its read in bits 0..30 (seqhash.c:184), isForward in bit 31
 *   dReadId[i] read ordinal (may be NULL; so may dPosF)
 * dCount: device U64[4] -> {number of modimizers found, overflow flag, fullest workgroup segment,
 * capacity to retry with}.  Workgroups stage their modimizers in per-workgroup segments of dWork
 * sized from `capacity`; when the flag is set (total > capacity, or one segment too small) the
 * outputs are unspecified, count is still the true total, and a retry with capacity = dCount[3]
 * succeeds.
 * dWork: mgScanWorkBytes(totalBases, nReads, capacity) bytes of device scratch. */
#define MG_POS_MASK 0x7fffffffu
#define MG_FWD_BIT  0x80000000u
size_t   mgScanWorkBytes (U64 totalBases, U32 nReads, U64 capacity) ;
MgStatus seqhashScanBatchDevice (const Seqhash *sh, const U32 *dPacked, U64 totalBases,
                                 const U64 *dReadOffsets, U32 nReads,
                                 U64 *dKmer, U32 *dPosF, U32 *dReadId, U64 capacity,
                                 U64 *dCount, void *dWork, void *stream) ;

/* Host-buffer convenience form of the above: bases[] as the reference's iterator takes them
 * (one byte per base, values 0..3), readOffsets[nReads+1].  Outputs are malloc()ed arrays the
 * caller frees; *survStart[nReads+1] gives each read's slice of the outputs. Returns the number of
 * modimizers, or -1 on error. */
int64_t seqhashScanBatch (const Seqhash *sh, const char *bases, const int64_t *readOffsets, int nReads,
                          U64 **kmer, int **pos, bool **isF, int64_t **survStart) ;

/* minimizerRCiterator + minimizerRCnext (seqhash.c:83-152) run to exhaustion on every read of a batch:
 * the (hash, pos | isF<<31) pairs successive minimizerRCnext calls return, reads in order, read r's at
 * [dReadStart[r], dReadStart[r+1]) (dReadStart holds nReads+1 entries).  One wavefront per read walks the
 * reference's chain of windows (see mg_minimizer.hip).  *n receives the total (also when it exceeds
 * `capacity`: MG_ERR_CAPACITY, nothing written). */
MgStatus seqhashMinimizerBatchDevice (const Seqhash *sh, const U32 *dPacked, U64 totalBases,
                                      const U64 *dReadOffsets, U32 nReads,
                                      U64 *dHash, U32 *dPosF, U64 *dReadStart, U64 capacity, U64 *n, void *stream) ;
/* host buffers in, malloc()ed arrays out (as seqhashScanBatch); returns the number of minimizers, -1 on error */
int64_t seqhashMinimizerBatch (const Seqhash *sh, const char *bases, const int64_t *readOffsets, int nReads,
                               U64 **hash, int **pos, bool **isF, int64_t **start) ;

/* Device modset (modset.c:45-62 as a batch).  The device table is created on first use from the
 * host arrays of `ms` and lives until modsetDestroy / mgModsetDeviceRelease.
 *
 * modsetAddBatchDevice: for i in order, what `index = modsetIndexFind (ms, kmer[i], true) ;
 * ++depth[index]` (modutils.c:25-26) would do: new k-mers receive indices max+1, max+2, ... in
 * order of first occurrence, ms->max is updated before return, depth increments accumulate on the
 * device until modsetSyncToHost.  dIndexOut (optional) receives the index of every kmer[i].
 * withDepth = 0 gives the modmap.c:109 form (insert without touching depth).
 *
 * modsetFindBatchDevice: `modsetIndexFind (ms, kmer[i], false)` — 0 for absent k-mers.
 *
 * n must be < 2^31 per call. */
MgStatus modsetAddBatchDevice (Modset *ms, const U64 *dKmer, U64 n, U32 *dIndexOut, int withDepth, void *stream) ;
MgStatus modsetFindBatchDevice (Modset *ms, const U64 *dKmer, U64 n, U32 *dIndexOut, void *stream) ;

/* Bring the host arrays of ms up to date with the device: value[] for new entries, saturating
 * depth[] += device counts (modutils.c:26), and (when wantIndex) the open-addressed index[] table
 * rebuilt exactly as the reference's sequence of inserts would have left it (modset.c:51-57). */
MgStatus modsetSyncToHost (Modset *ms, int wantIndex) ;
int      mgXferThreadCount (void) ;         /* host threads that move whole arrays between the device and the Modset's own arrays (modsetSyncToHost, device rebuilds): 4 (measured best: tools/xfer_probe.py) or fewer if the process may use fewer CPUs; MODGPU_XFER_THREADS overrides, up to 16 */
/* What that team has done on the current device since the process started (tests, diagnostics; nothing resets it, so a caller takes
 * differences).  out8 (host): [0] transfers run, [1] pieces moved, [2] threads of the last transfer, [3] bytes per piece in force
 * (MODGPU_XFER_PIECE_KB), [4] uploads of a mostly untouched array that went by the page map (only the pages ever written are read
 * and sent), [5] such uploads that took the plain copy instead, [6] runs of pages the last of them sent, [7] bytes it did not send. */
void     mgXferDiag (U64 out8[8]) ;
/* Drop the device table (host arrays untouched; pending device depth counts are synced first). */
MgStatus mgModsetDeviceRelease (Modset *ms) ;
/* Tell the library the caller changed ms->value/max/depth on the host behind its back. */
void     mgModsetHostChanged (Modset *ms) ;
/* Forget every entry: the state modsetCreate (modset.c:15-31) returns, without reallocating.
 * Clears the device table (if any), ms->max, and the host index[]/depth[]/info[] of used entries. */
MgStatus mgModsetClear (Modset *ms, void *stream) ;

/* Slots of the device table behind ms (0 when there is none): what bench.py prices the bucket image with. */
U64 mgModsetDeviceSlots (Modset *ms) ;

/* A check of the device table's layout that does not use the lookups (tests, diagnostics).  out6 (host): [0] keys whose path from
 * their home slot to their own crosses an empty slot, [1] keys in a bucket other than the one they imply, [2] keys held twice in a
 * bucket -- all 0 in a sound table -- [3] keys in the table; and, since the device table was made, [4] buckets the build laid out by
 * prefix scan, [5] those of them whose entries ran over the bucket's end and came in again at its first slot. */
MgStatus mgTableCheckLayout (Modset *ms, U64 *out6) ;
/* Which geometry the device table behind ms has and which kernels have run on it (tests, diagnostics).  out9 (host): [0] log2 of the
 * number of buckets, [1] slots per bucket; and, counted since the device table was made: lookup batches answered [2] by direct probes,
 * [3] by one partition level, [4] by two levels over the 16-byte slots, [5] by two levels over the 8-byte copy, [6] times that copy was
 * made, [7] changes of geometry done bucket by bucket, [8] those done with global atomics.  [2] also counts every chunk of an add that
 * returns indices (modsetAddBatchDevice with dIndexOut, mgInsertReadsDevice): it finds them by the same direct probes.  All 0 when ms
 * has no device table (this call makes none). */
MgStatus mgTableDiag (Modset *ms, U64 *out9) ;
/* Which instance of the scan kernel has run (tests, diagnostics): launches since the process started, counted where the instance is
 * chosen; nothing resets them, so a caller takes differences.  The hit test has six modes -- 0 any d (64-bit inverse), 1 d a power of
 * two (mask), 2 the low-bits filter for powers of two, 3 odd d (64-bit), 4 odd d in 32-bit arithmetic, 5 any d in 32-bit arithmetic --
 * and out18 (host) holds: [2 * mode + where] launches of the batch scan, where = 1 when positions or read ids were asked for and 0
 * for the k-mers alone; [12 + mode] launches of the per-read iterator's kernel. */
MgStatus mgScanDiag (U64 *out18) ;
/* Which threshold test the low-bits filter (mode 2 above) has run with (tests, diagnostics): launches since the process started, batch
 * scan and iterator alike, counted where the instance is chosen, out2 (host): [0] with four starts' top bytes packed into one register
 * and tested together (d <= 256; MODGPU_SCAN_PACKED_TEST=0 turns it off), [1] with every start compared on its own.  Their sum is what
 * mgScanDiag counts for mode 2.  Nothing resets them: take differences. */
MgStatus mgScanTailDiag (U64 *out2) ;
/* The packed test itself, on the host (tests): bit 8j + 7 of the result is set when byte j of acc is below N, for nRep = 0x01010101 * N,
 * 1 <= N <= 32 -- and for a byte equal to N directly above a flagged byte, which the filter, a superset test, may pass.  The line the
 * kernel compiles (csrc/mg_packedtest.h). */
U32 mgScanBytesBelow (U32 acc, U32 nRep) ;
/* Where the bucketed add's value writer has run (tests, diagnostics): launches since the process started, out2 (host): [0] on the set's own
 * stream, behind the add's merge kernel and beside whatever the caller starts next, [1] on the caller's stream inside the add
 * (MODGPU_VALUE_ASYNC: 0 always there, 1 never, unset: off the caller's stream for mgAddReadsDevice).  Nothing resets them: take differences. */
MgStatus mgValueWriterDiag (U64 *out2) ;

/* modutils.c:53-63 on the device: dHist[65536] (U64) += histogram of depth[1..max], where depth is
 * the host depth at last sync plus pending device counts, saturated at 65535. */
MgStatus modsetDepthHistogramDevice (Modset *ms, U64 *dHist65536, void *stream) ;

/* One-call forms used by the drivers and the benchmark: scan a device-resident packed batch and
 * feed the modimizers straight into the modset.
 *   mgAddReadsDevice   = addSequence (modutils.c:19-31) over every read of the batch;
 *   mgQueryReadsDevice = the lookup loop of queryProcess (modmap.c:197-206): seeds (index,pos)
 *                        per read incl. misses.
 * nHash receives the number of modimizers.  Scratch is taken from an internal per-modset arena
 * that grows on demand (two of them, used in turn, when a set takes one mgAddReadsDevice after
 * another: the last step of an add -- writing the set's value[] on the device -- runs on a stream
 * of the library's own and may still be running when the call returns, beside whatever the caller
 * starts next; every call of this library that looks at the values waits for it, and a device-wide
 * synchronize covers it.  MODGPU_VALUE_ASYNC=0 keeps that step inside the call). */
MgStatus mgAddReadsDevice (Modset *ms, const U32 *dPacked, U64 totalBases,
                           const U64 *dReadOffsets, U32 nReads, U64 *nHash, void *stream) ;
MgStatus mgQueryReadsDevice (Modset *ms, const U32 *dPacked, U64 totalBases,
                             const U64 *dReadOffsets, U32 nReads,
                             U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity,
                             U64 *nSeeds, void *stream) ;

/* mgQueryReadsDevice in two halves, for batches that follow one another (config 3: 90 Gbp of reads in batches of 10): Async starts the
 * batch's scan on a stream of the library's own, into the other of two scratch arenas, and returns at once; Wait runs the lookups on
 * `stream` and returns when the seeds are complete.  Called as   Async (0); for every i: { Async (i + 1); Wait (i); }   the scan of batch
 * i + 1 (bound by instruction issue) runs beside the lookups of batch i (bound by memory requests).  At most two batches in flight,
 * waited for in the order they were started, each with output arrays of its own; the batch on `stream` must be complete there when
 * Async is called (the scan waits for what that stream holds at that moment); until the last ticket has been waited for the modset takes
 * no other batch call (they fail with MG_ERR_ARG).  The results are those of mgQueryReadsDevice, bit for bit. */
MgStatus mgQueryReadsDeviceAsync (Modset *ms, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                  U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity, void **ticket, void *stream) ;
MgStatus mgQueryReadsDeviceWait (void *ticket, U64 *nSeeds, void *stream) ;      /* frees the ticket, also on error */

/* mgInsertReadsDevice = the insert loop of referenceFastaRead (modmap.c:106-118, isAdd true): every
 * modimizer is inserted WITHOUT touching depth and its (index,pos,read) returned. */
MgStatus mgInsertReadsDevice (Modset *ms, const U32 *dPacked, U64 totalBases,
                              const U64 *dReadOffsets, U32 nReads,
                              U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity,
                              U64 *nSeeds, void *stream) ;

/* modsetMerge (modset.c:106-128) with the second set given as bare arrays, entries at [1..n2]: merging
 * per-GPU modsets in rank order reproduces the single-stream build exactly. */
bool mgModsetMergeArrays (Modset *ms1, U64 *value2, U16 *depth2, U8 *info2, U32 n2) ;
/* The same with the arrays in DEVICE memory, entry i at [i - 1], and ms1 on the device: nothing of the second set crosses the host
 * link (what mgModsetMergeRankOrder does with what its peers sent).  false = ms1 has no device table, nothing done. */
bool mgModsetMergeDeviceArrays (Modset *ms1, const U64 *dValue2, const U16 *dDepth2, const U8 *dInfo2, U32 n2) ;

/* Multi-GPU from C, straight on RCCL (BASELINE config 4).  Reads shard over the GPUs, every GPU builds its own modset, no
 * collective on the data path; these are the exchanges there are.  Communicators as RCCL has them: ONE PROCESS, N DEVICES, a host
 * thread per device (mgCommInitAll; each thread calls mgSetDevice (device of its comm) and then uses the library as on one GPU) -- or ONE
 * PROCESS PER DEVICE (rank 0 calls mgCommGetUniqueId and hands the 128 bytes to the others by its own means -- a file, a socket, MPI --,
 * every rank calls mgCommInitRank).  librccl is loaded by the first of these calls, not before. */
typedef struct MgComm MgComm ;
MgStatus mgCommInitAll (MgComm **comms /* [nDev] out */, int nDev, const int *devices /* 0: 0 .. nDev-1 */) ;
MgStatus mgCommGetUniqueId (void *id128) ;
MgStatus mgCommInitRank (MgComm **comm, int nRanks, int rank, const void *id128, int device) ;
int      mgCommRank (const MgComm *c) ;
int      mgCommSize (const MgComm *c) ;
void     mgCommDestroy (MgComm *c) ;
/* config 4's collective: hist65536[d] (host, U64) = over all ranks, the number of modset entries of depth d (modutils.c:53-63 per rank,
 * all-reduced with SUM: 512 KiB a rank over xGMI).  Every rank calls it with its own set and gets the sum. */
MgStatus mgHistogramAllReduce (Modset *ms, U64 *hist65536, MgComm *c) ;
/* reads counted against a FIXED set that every rank holds (the same entries everywhere; modasm.c:158-174: depth zeroed, ++depth per hit,
 * saturating): depth[i] = min (65535, sum over the ranks of their depth[i]) on every rank, in ms->depth and in the device table.  Exact: a
 * saturating add is associative.  4 bytes per entry per rank through one ncclAllReduce (sum, uint32). */
MgStatus mgDepthAllReduce (Modset *ms, MgComm *c) ;
/* the exact global set: on rank `root` ms becomes the merge of every rank's set in RANK order with modsetMerge semantics
 * (modset.c:106-128): with contiguous blocks of reads per rank and root = 0 that is, bit for bit, the set one stream over all the reads
 * builds.  Every rank calls it; the others' sets are sent (point to point, one rank at a time) and left as they are. */
MgStatus mgModsetMergeRankOrder (Modset *ms, MgComm *c, int root) ;

/* Host-side batch mirrors of the reference callers' loops. */
/* modutils.c:19-31 over nReads reads; returns total hashes, -1 on error. ms->max updated. */
int64_t mgAddSequenceBatch (Modset *ms, const char *bases, const int64_t *readOffsets, int nReads) ;
/* modutils.c:53-63 */
void    mgDepthHistogram (Modset *ms, FILE *f) ;
/* modutils.c:33-51 on reads already in memory: adds every read, prints the "added ..." line */
int     mgAddSequences (Modset *ms, const char *bases, const int64_t *readOffsets, int nReads, FILE *out) ;
/* modutils.c:194-198 ("-wt") */
void    mgModsetWriteText (Modset *ms, FILE *f) ;

/* modmap.c's Reference (modmap.c:35-47) and its three operations, on sequences already in memory
 * (bases 0..3 one byte each, offsets[n+1], names[n]).  The per-k-mer loops run on the GPU
 * (mgInsertReadsDevice / mgQueryReadsDevice), and so do the per-occurrence bookkeeping, the copy classes and
 * the CSR pack (modmap.c:106-134,74-91: ordered append, exclusive scan, stable sort by index) and the queries'
 * tallies and seed chaining (modmap.c:213-276); the arrays below are the caller's, filled from the device when
 * mgReferenceRead / mgReferenceFastaRead return; the host formats the Q / M lines. */
typedef struct {
  Modset *ms ;
  U32 size ;                   /* capacity of index/offset/id */
  U32 max ;                    /* occurrences stored */
  U32 *index, *offset, *id ;   /* per occurrence: modset index, position in its sequence, sequence id */
  U32 *depth ;                 /* occurrences per modset index */
  U32 *rev, *loc ;             /* CSR inverse: occurrences grouped by modset index */
  int nSeq ;
  char **names ;               /* sequence names (the reference keeps them in a DICT) */
  U32 *len ;
} MgReference ;
MgReference *mgReferenceCreate (Modset *ms, U32 size) ;                               /* modmap.c:49-64 */
void mgReferenceDestroy (MgReference *ref) ;                                          /* modmap.c:66-72 */
/* modmap.c:93-134: scan + insert/lookup every sequence, classify copy number, pack; prints the two
 * report lines to out.  Returns 0 on success. */
int  mgReferenceRead (MgReference *ref, const char *bases, const int64_t *offsets, int nSeq,
                      const char **names, bool isAdd, FILE *out) ;
/* modmap.c:136-182: <root>.mod + <root>.ref in the reference's on-disk format (gzip streams, as its
 * fzopen writes them; gzip or plain accepted on read), interchangeable with modmap -w / -r.
 * mgReferenceLoad also creates the Modset (ref->ms, with its own Seqhash) as referenceRead does; as in the
 * reference, mgReferenceDestroy leaves ref->ms alone (modmap.c:66-72): the caller destroys it, and its hasher. */
void mgReferenceWrite (MgReference *ref, const char *root) ;
/* What the library's writers (mgReferenceWrite, mgReadsetWrite) put between themselves and the disk, for a caller's own modsetWrite
 * (modset.c:79-88 takes any FILE *): the bytes written to the returned FILE * become a gzip file of independent members of 16 MiB,
 * deflated by a team of threads (MODGPU_GZIP_THREADS; default: the CPUs the process may use) and written in order.  gzread -- the
 * reference's fzopen "r" (utils.c:107-127) -- and gunzip read such a file as the one stream the reference's single gzwrite would have
 * made; fclose () finishes it.  0 if `name` cannot be created. */
FILE *mgGzipOpenWrite (const char *name) ;
/* ... and its counterpart for modsetRead (modset.c:90-104): every member the writer makes carries its compressed and uncompressed size
 * in a gzip extra field (RFC 1952 2.3.1.1, subfield 'M' 'G'; gzread and gunzip skip it), so the members are found without inflating
 * anything and inflated by the team -- whole members straight into the array a large fread hands over.  0 if `name` is not such a file
 * from its first byte to its last (any other gzip file, a plain file): the caller then takes the reference's fzopen / gzopen, as
 * mgReferenceLoad and mgReadsetLoad do by themselves. */
FILE *mgGzipOpenRead (const char *name) ;
/* the reference's fzopen (utils.c:107-127) on top of the two: "w" = mgGzipOpenWrite; "r" = mgGzipOpenRead, and for any other gzip file
 * or a plain file zlib's gzopen behind a FILE * (what modsetRead / modsetWrite, seqhashRead / seqhashWrite take). */
FILE *mgFzOpen (const char *name, const char *mode) ;
MgReference *mgReferenceLoad (const char *root) ;
/* modmap.c:188-281: "Q" line and "M" lines for every read. */
int  mgQueryProcess (MgReference *ref, const char *bases, const int64_t *offsets, int nReads,
                     const char **names, FILE *out) ;
/* modmap's -v toggle (modmap.c:23,348): with it on, mgQueryProcess / mgQueryFile also print the per-seed lines of
 * modmap.c:218-229 ("  <pos>\t<seq> <offset>[\t<seq2> <offset2>]", to stdout as the reference's printf does,
 * before the M line a seed closes); the seed lists then come back to the host and are chained there. */
void mgSetVerbose (int on) ;

/* modasm's long-read set (modasm.c:30-57,79-86) as readsetFileRead + invBuild leave it:
 * per read its length, hit / miss counts and copy-class tallies; the hits (modset index, bit 31 =
 * forward) with the 16-bit distance to the previous hit; per mod the reads that hit it.  Reads are
 * numbered from 1 as in the reference; the scan + lookup of every read is one GPU batch call. */
typedef struct {
  Modset *ms ;
  int nReads, capReads ;
  int *len, *nHit, *nMiss ;     /* [1..nReads] */
  int (*nCopy)[4] ;             /* [1..nReads]: hits on copy 0 / 1 / 2 / M mods */
  U64 *hitStart ;               /* hits of read i: hit/dx[hitStart[i] .. hitStart[i+1]) */
  U32 *hit ; U16 *dx ;
  U64 totHit, capHit ;
  U64 *invStart ;               /* [ms->max+2]: mod i is hit by the reads invSpace[invStart[i] .. invStart[i+1]) */
  U32 *invSpace ;               /* (one entry per hit, read order; none for mods whose depth saturated, modasm.c:266,278) */
  U8 *bad ; int *contained ;    /* [1..nReads]: Read.bad (bits from 1: badRepeat, badOrder10, badOrder1, badNoMatch, badLowHit, badLowCopy1; modasm.c:36-46) and Read.contained, as
                                   the overlap passes below leave them; zero after create and ingest, kept by mgReadsetLoad / mgReadsetWrite */
} MgReadset ;
MgReadset *mgReadsetCreate (Modset *ms) ;                                                   /* modasm.c:90-98 */
void mgReadsetDestroy (MgReadset *rs) ;
/* modasm.c:151-191 + 258-287: depth[] is rebuilt from these reads (modasm.c:158) */
int  mgReadsetRead (MgReadset *rs, const char *bases, const int64_t *offsets, int nReads) ;
int  mgReadsetFileRead (MgReadset *rs, const char *filename) ;
void mgReadsetStats (MgReadset *rs, FILE *out) ;                                            /* modasm.c:193-253 */
void mgReadsetWrite (MgReadset *rs, const char *root) ;                                     /* modasm.c:108-126 */
MgReadset *mgReadsetLoad (const char *root) ;                                               /* modasm.c:128-149; creates rs->ms, which mgReadsetDestroy leaves to the caller (modasm.c:100-107) */
/* modasm -C (cleanMods, modasm.c:514-555): the repeat / internal / minor-variant flags of every mod from the reads' hit lists, OR-ed into
 * ms->info (what is set stays set); rs->nCopy and the inverse lists as its invBuild leaves them (modasm.c:552); the line "set %d repeated,
 * %d internal, %d minor_variant mods" to `out`.  As in the reference (modasm.c:522-523) the LAST read contributes no flag.  The hits are
 * sorted by mod on the device; a set of 2^32 - 16 hits or more, or a device without room for it, takes host loops that give the same bytes.
 * 0, or -1 with mgLastError ().  ...Path: what the calling thread's last call took: 0 = the device, 1 = the host loops, -1 = it failed before. */
int  mgReadsetCleanMods (MgReadset *rs, FILE *out) ;
int  mgReadsetCleanModsPath (void) ;
/* modasm -P (readProperties, modasm.c:912-952): per read (the last one included) how its copy-1 mods repeat in it: the "MT" lines of the
 * read in ascending mod order, its "READ" line, its "RM" line if it has one.  ms and rs are not modified.  Paths and result as above. */
int  mgReadsetProperties (MgReadset *rs, FILE *out) ;
int  mgReadsetPropertiesPath (void) ;
/* modasm's overlap passes: -o1 / -o2 / -b / -c are all findOverlaps (modasm.c:314-418).  What it works out for a query read x and a partner y that
 * shares at least 3 of x's copy-1 mods -- nHit, the relative strand, the order and flip counts, containment -- depends on the two hit lists and on
 * ms->info / ms->depth alone, and is made for a batch of queries at once on the device (mg_overlap.hip); what depends on the order of the calls -- a
 * partner whose `bad` is set NOW is skipped, the query's own badRepeat / badNoMatch / badLowHit / badLowCopy1 -- is replayed on the host, query by
 * query in the order given.  The list of x: the partners (x itself among them) by nHit descending, equal nHit in order of arrival.
 *   mgReadsetFindOverlaps   findOverlaps (x, level) for x = reads[0 .. n): level 1 prints the "RR" line, 2 the "RH" lines too (-o1 i is one read at
 *                           level 2).  res != 0: the lists as -b / -c see them (a skipped partner has flags 4 and zero counts); free with mgOverlapsFree.
 *   mgReadsetOverlapStats   -o2 d: level 1 for x = d, 2d, ... (d >= 1)
 *   mgReadsetMarkBadReads   -b (markBadReads, modasm.c:1266-1322): clears every `bad`, then sets them; the three "MB" lines
 *   mgReadsetMarkContained  -c (markContained, modasm.c:1370-1394): sets `contained` (never reset); the "MC" line
 * Every line goes to `out` (0: none), those the reference printf ()s included.  0, or -1 with mgLastError (): a read number outside 1 .. nReads, a
 * read of more than 65534 hits (the reference's U16 hmap / nHit wrap), a copy-1 mod of a query whose depth saturated (it has no inverse list, and
 * the reference reads through a null pointer); nothing has been replayed then unless a batch was done before.  A set of 2^32 - 16 hits or more,
 * MODGPU_READSET_HOST=1 or a device without room take host loops that give the same records.  ...Path: as above.  ...Diag: the calling thread's last
 * call: batches, candidates (entries of the inverse lists walked), pairs kept (nHit >= 3), launches of the pair kernel. */
typedef struct { U32 n ; U64 *start ;              /* [n+1]: entries of query q at [start[q], start[q+1]) */
                 U32 *iy ; U16 *nHit, *nBadOrder, *nBadFlip ; U8 *flags ; } MgOverlaps ;   /* flags: 1 isPlus, 2 isContained, 4 skipped (y was bad) */
int  mgReadsetFindOverlaps (MgReadset *rs, const U32 *reads, U32 n, int level, FILE *out, MgOverlaps *res /* may be 0 */) ;
void mgOverlapsFree (MgOverlaps *res) ;
int  mgReadsetOverlapStats (MgReadset *rs, U32 d, FILE *out) ;      /* -o2 d */
int  mgReadsetMarkBadReads (MgReadset *rs, FILE *out) ;             /* -b: the three MB lines */
int  mgReadsetMarkContained (MgReadset *rs, FILE *out) ;            /* -c: the MC line */
int  mgReadsetOverlapsPath (void) ;                                 /* 0 device, 1 host loops, -1 failed before */
void mgReadsetOverlapsDiag (U64 out4[4]) ;                          /* last call of this thread: batches, candidates, pairs kept, pair-kernel launches */
/* modasm -R <ref> / -T <min> <max> / -rb <n>: the rDNA flags of the mods and their LD test (refFlag, modasm.c:752-860; testMods, 595-748; resetBits,
 * 864-908).  One pipeline: -R makes the per-mod ModInfo, which is in no file, and -T and -rb are its only readers, so all three run in one process.
 * ModInfo, the reads' otherFlags byte (bit 1 = isRDNA) and the count of -T calls live beside the set (MgReadset has no field for them) and go with
 * mgReadsetDestroy; mgReadsetWrite / mgReadsetLoad keep otherFlags (byte 25 of the 72-byte record), ModInfo and the count do not survive a file.
 *   mgReadsetRefFlagHits   refFlag from the reference sequences' hits in file order (index[j] in 1 .. ms->max at position pos[j]; misses left out):
 *                          the last hit of a mod wins rDNApos; per read the 200th core-and-ref hit from either end (mg_rdna.hip); the walk between the
 *                          two, which depends on the order of the reads, on the host; the five counting lines (modasm.c:855-859)
 *   mgReadsetRefFlagFile   -R: the file through the set's hasher and the device lookups (as mgRefPaintFile: N is base 0), then the above.  The
 *                          reference maps N to 0 only after a -f in the same process and otherwise hashes a base 4 that its tables do not have
 *   mgReadsetResetBits     -rb op, ops 1 2 3 as they stand (any other: no line, 0); nCopy[] rebuilt.  -1 without -R; -1 for op 3 on an empty set
 *   mgReadsetTestMods      -T: per tested mod i (minDepth <= depth < maxDepth, RDNA and not REPEAT, not copy 0) and partner mod m of the same kind the
 *                          count and the least and greatest signed distance over the reads that hold i (mg_rdna.hip: the reference's sort is not
 *                          needed); the rules of modasm.c:658-705 per (i, m) on the device, the closing loop (708-740), "YY-TEST" lines into yFile
 *                          and the "RUN" line into out on the host, the "ZZ-TEST" lines into zFile only if it is given.  -1, nothing modified, where
 *                          the reference breaks: no -R yet ("need to run -R first"); a tested mod of depth 0 or 65535; a visit that would count
 *                          before its array (len - x - w < 0) or look beyond it: none can happen with w <= k; a -T that tests no mod (the reference
 *                          dies at its end: arrayDestroy (0)); a second tested mod whose start or end array passes 20000 cells (the reference
 *                          clears 20000 cells between tested mods, array.c:103, and counts on stale sums beyond: reads of more than ~20 kb)
 * Host loops give the same bytes for a set of 2^32 - 16 hits or more, MODGPU_READSET_HOST=1 or a device without room, and for a -T that walks fewer
 * than 2^21 hits (the visited reads' hit counts together; MODGPU_READSET_HOST=0 sends it to the device).  info[] changed: the calls end in
 * mgModsetHostChanged.  ...RdnaPath: the calling thread's last call: 0 device, 1 host loops, -1 failed before.  ...RdnaDiag: its last -T: batches of
 * tested mods (MODGPU_TESTMODS_BATCH mods per batch; unset: by the free device memory), tested mods, visits, partner occurrences.  ...RdnaGrid: what
 * its last -T on the device launched: tiles of partner ordinals, the least and the greatest share of the visits over its batches, cells per count
 * array (the longest read + 1); zeros after the host loops. */
typedef struct { U8 flags ; /* 1 isRefRDNA, 2 isCoreRDNA, 4 isVarRDNA, 8 isMultiRDNA (modasm.c:61-77) */
                 int rDNApos, nGood, nMod2, nBadLD, nSplit, nSplitLD ; } MgModInfo ;
int  mgReadsetRefFlagFile (MgReadset *rs, const char *refFile, FILE *out) ;
int  mgReadsetRefFlagHits (MgReadset *rs, const U32 *index, const int *pos, U64 n, FILE *out) ;
int  mgReadsetResetBits (MgReadset *rs, int op, FILE *out) ;
int  mgReadsetTestMods (MgReadset *rs, int minDepth, int maxDepth, FILE *yFile, FILE *zFile, FILE *out) ;      /* yFile / zFile / out may be 0 */
const MgModInfo *mgReadsetModInfo (const MgReadset *rs) ;           /* [ms->max+1], 0 before -R */
const U8 *mgReadsetReadFlags (const MgReadset *rs) ;                /* [1..nReads]: Read.otherFlags, bit 1 = isRDNA */
int  mgReadsetTestModsRun (const MgReadset *rs) ;                   /* -T calls made on this set: the reference's static RUN */
int  mgReadsetRdnaPath (void) ;
void mgReadsetRdnaDiag (U64 out4[4]) ;
void mgReadsetRdnaGrid (U32 out4[4]) ;

/* modrep -R <ref.fa> <ref.mod> -s3 <reads.fa> <reads.mod> (modrep.c:27-63,170-268; the rest of that file is its "OLD VERSIONS").
 * Scan, lookups and every per-read and per-mod reduction run on the device (mg_modrep.hip); the host formats the lines.  All of these
 * need a HIP device: there is no host fallback.
 *
 * MgRepRef is modrep.c:20-25 as refCreate leaves it: for every entry of ms found in the one reference sequence pos[index] = the position
 * of its LAST occurrence and isF[index] its strand there (entries not found: 0 / false); len = the largest position + 1 (0: none found).
 * refCreate dies when it meets an entry whose pos[] is already non-zero (modrep.c:48), so an occurrence at position 0 does not protect
 * its entry: a mod may occur once, or twice if its first occurrence is at position 0.  Both creators print modrep.c:58-59 ("found %d of
 * %d locations in ref length %llu") to err (0: not printed) and return 0 with mgLastError () holding the program's message otherwise:
 * "duplicate mod entry at position %d in ref", "multiple sequences in ref file - only one allowed", and those of unreadable files. */
typedef struct {
  Modset *ms ;
  int len ;
  int *pos ;                    /* [ms->max + 1] */
  bool *isF ;                   /* [ms->max + 1] */
  int ownsMs ;                  /* mgRepRefCreate read ms itself: mgRepRefDestroy destroys it and its hasher */
} MgRepRef ;
/* modrep.c:27-63: the .mod through mgFzOpen (gzip or plain), the FIRST record of seqFile with N / n read as A (modrep.c:559) */
MgRepRef *mgRepRefCreate (const char *seqFile, const char *modFile, FILE *err) ;
/* modrep.c:43-54 on a sequence in memory (bases 0..3); ms stays the caller's */
MgRepRef *mgRepRefFromArrays (Modset *ms, const char *bases, int64_t len, FILE *err) ;
void mgRepRefDestroy (MgRepRef *ref) ;

/* analyzeSequences3 (modrep.c:170-268) for a file that comes in batches.  ms is the SECOND set (the .mod given to -s3); the reads are
 * scanned with the REFERENCE set's hasher both times, as the program does, so the two sets must have one k.
 *   per read (modrep.c:193-209): its first 100 modimizers found in ref->ms vote, seqF for the reference's strand and seqR against; the
 *     read is bad when n < 100 || (seqF > 10 && seqR > 10) and prints "BADREAD %5d len %5d n %d F %4d R %4d";
 *   a good read with seqF < seqR is reverse-complemented (modrep.c:215-221), scanned again and its modimizers looked up in ms
 *     (modrep.c:223-233): hits (k = index, x = position in the ORIENTED read), ++n[k], ++nPre[k] for the second and later hit on k of a read;
 *   after the file (modrep.c:236-258): over i = 0 .. max - 1 (entry 0 counted, entry max not: the program's arrays end there) nPre[i] != 0
 *     counts as dup, adds to tDup and sets n[i] = 0, anything else counts as good; minMax folds max_r = the largest n[k] over a good
 *     read's hits with `if (!minMax || max_r < minMax) minMax = max_r`, so a read with max_r == 0 starts the fold again.
 * The library's arrays have max + 1 entries and tally entry max like any other (the program writes past its arrays there).
 * The hits' k, x and read stay on the device from a batch to the end: n[] and nPre[] are final only then. */
typedef struct MgRepRun MgRepRun ;
typedef struct {
  int nRead, nBad, nGood ;                   /* modrep.c:236 */
  int *n, *seqF, *seqR ;                     /* [nRead]: modrep.c:196-202 */
  bool *bad, *isF ;                          /* [nRead]: modrep.c:204; isF = good and not reverse-complemented (modrep.c:221) */
  U32 max ;                                  /* ms->max */
  int *modN, *modNPre ;                      /* [max + 1]: mods[].n (zeroed where nPre, modrep.c:242) and mods[].nPre */
  int *goodI, *goodLen ;                     /* [nGood]: Read.i (the read's ordinal from 0), Read.len */
  U64 *hitStart ;                            /* [nGood + 1]: good read g's hits are hitK / hitX [hitStart[g] .. hitStart[g + 1]) */
  int *hitK, *hitX ;
  int nMod, nDup, tDup, minMax ;             /* modrep.c:237-246,250-258 */
} MgRepResult ;
void mgRepResultFree (MgRepResult *res) ;    /* the arrays (malloc); res itself is the caller's */
MgRepRun *mgRepRunBegin (MgRepRef *ref, Modset *ms) ;                          /* modrep.c:186-191; 0 = error */
/* modrep.c:192-234 for a batch (bases 0..3, offsets[nReads + 1]): its BADREAD lines to out in read order; read numbers go on from the call before.  0 / -1 */
int  mgRepRunAdd (MgRepRun *run, const char *bases, const int64_t *offsets, int nReads, FILE *out) ;
/* modrep.c:236-258: the two lines to err (0: not printed), the results into res (0: not wanted); frees the run, also on error.  0 / -1 */
int  mgRepRunFinish (MgRepRun *run, FILE *err, MgRepResult *res) ;
/* modrep.c:170-268 from files: the .mod through mgFzOpen, the reads in batches through mgSeqOpen / mgSeqNextBatch (N read as A).  0 / -1 with
 * the program's message ("failed to open mod file %s", "failed to read modset from file %s", "can't open sequence file %s") */
int  mgRepAnalyze3File (MgRepRef *ref, const char *seqFile, const char *modFile, FILE *out, FILE *err, MgRepResult *res) ;
int  mgRepPath (void) ;                      /* test hook: the calling thread's last run (-s3, -s1 or -s2): 0 = finished through the device kernels, -1 = it failed or none ran */

/* modrep -s1 <reads.fa> <reads.mod> (analyzeSequences1, modrep.c:272-489) and -s2 (analyzeSequences2, modrep.c:493-539) on the device
 * (mg_modrep1.hip).  -s1's per-read pass is -s3's without the BADREAD lines (modrep.c:305-310 print nothing) and without the per-read
 * duplicate array: the same MgRepRun, mgRepRunAdd called with out = 0.  The end of the file (modrep.c:354-480) runs in kernels:
 *   cleanMods, five times (modrep.c:354,370,392,424,446), each printing "NMOD mod0 %d modSmall %d modBig %d modGood %d": over
 *     i = 0 .. max - 1, n[i] < 5 and n[i] > reads / 2 are zeroed, then the hits on mods with n == 0 leave the reads;
 *   the run removal (modrep.c:356-369): in a read a hit stays if x >= xNext, then xNext = x + k; the others take 1 from their mod's n;
 *   buildPrePost, four times (modrep.c:373,395,427,449): every pair of neighbouring hits of a read is a link (k0, k1, dx); mod k0's post
 *     list gets (k1, n, x = sum of dx), mod k1's pre list (k0, n, x), nPost[k0] and nPre[k1] count the links.  addHit (modrep.c:129-148)
 *     moves an entry to the front when its count passes the front's; the order that leaves is computed in closed form;
 *   the mod verdicts (modrep.c:374-391,428-445), which read pre[0] of an EMPTY pre list, too: what the last non-empty build left there;
 *   the weak links (modrep.c:395-415): a read with a link that fewer than 5 reads share leaves, "reduced %d reads to %d reads" goes to err;
 *     then n[] is counted again over every hit of a read but its last (modrep.c:417-423);
 *   the report (modrep.c:449-480): "MOD .." per surviving mod, the reads sorted by their k sequences (readOrder; equal reads stay in input
 *     order, as glibc's merge sort leaves them), "READ .." per read and "BLOCK .." after every block of equal reads but the last.
 * The program's array of mods has max entries and is indexed by entries up to max: a file in which entry max of the second set occurs in
 * a read is refused (-1, mgLastError () says so, nothing is printed).  err gets "read %d reads, %d bad, %d good: " and a newline where
 * the program writes its timing. */
typedef struct {
  int nRead, nBad, nGood ;                   /* modrep.c:351 (0 from mgRepAnalyze1Hits but nGood) */
  U32 max ;                                  /* ms->max */
  int nmod[5][4] ;                           /* the five NMOD lines: mod0, modSmall, modBig, modGood */
  int readsBefore, readsAfter ;              /* modrep.c:414 */
  int *modN, *modNPre, *modNPost ;           /* [max + 1]: mods[].n, nPre, nPost as the report finds them */
  U64 *preStart, *postStart ;                /* [max + 2]: mod i's lists are pre* [preStart[i] .. preStart[i + 1]) and post* likewise, in list order */
  int *preK, *preN, *preX, *postK, *postN, *postX ;      /* Hit.k (the partner), Hit.n, Hit.x */
  int *readI ;                               /* [readsAfter]: Read.i of the surviving reads, sorted (modrep.c:463) */
  U64 *hitStart ;                            /* [readsAfter + 1]: sorted read r's mods are hitK [hitStart[r] .. hitStart[r + 1]) */
  int *hitK ;
} MgRep1Result ;
void mgRep1ResultFree (MgRep1Result *res) ;  /* the arrays (malloc); res itself is the caller's */
/* modrep.c:351-480 for a run whose batches were added with out = 0: the lines to out and err (0: not printed), the results into res
 * (0: not wanted); frees the run, also on error, as mgRepRunFinish does.  0 / -1 */
int  mgRepRunFinish1 (MgRepRun *run, FILE *out, FILE *err, MgRep1Result *res) ;
/* modrep.c:272-489 from files, as mgRepAnalyze3File */
int  mgRepAnalyze1File (MgRepRef *ref, const char *seqFile, const char *modFile, FILE *out, FILE *err, MgRep1Result *res) ;
/* the file's end alone (modrep.c:354-480) on hit lists the caller holds: read r (Read.i = readI[r]) has the hits hitK / hitX
 * [hitStart[r] .. hitStart[r + 1]), 1 <= k <= max, 0 <= x; K: the hasher's k.  Uploads them and runs the kernels.  0 / -1 */
int  mgRepAnalyze1Hits (U32 max, int K, int nReads, const int *readI, const U64 *hitStart, const int *hitK, const int *hitX,
                        FILE *out, FILE *err, MgRep1Result *res) ;
/* modrep.c:520-535 for a batch (bases 0..3, offsets[nReads + 1]): the reads as they are, scanned with the reference set's hasher; a read that
 * holds the reference's entries 1 and 961 adds to counts4[0], 961 and 1951 to [1], 1951 and 2961 to [2], 2961 and 1 to [3].  0 / -1 */
int  mgRepCount2 (MgRepRef *ref, const char *bases, const int64_t *offsets, int nReads, int counts4[4]) ;
/* modrep.c:498-539 from files: counts4 is zeroed, "n1 %d n2 %d n3 %d n4 %d" goes to out (0: not printed).  The second .mod file is opened
 * and read as the program does (and fails with its messages); nothing else is done with it */
int  mgRepAnalyze2File (MgRepRef *ref, const char *seqFile, const char *modFile, FILE *out, int counts4[4]) ;
/* test hook: the calling thread's last -s1 end: [0] builds made, [1] links of the largest build, [2] entries of its post lists, [3] hits
 * removed as runs, [4] reads removed for weak links, [5] mods whose verdict read a pre[0] that an earlier build had left (the list
 * being empty now), [6] kernels launched, [7] 0 */
void mgRep1Diag (U64 out8[8]) ;

/* The file front end (seqio.c:30-346 for FASTA / FASTQ text, plain, gzip or blocked gzip, with the callers'
 * dna2indexConv + N->0 conversion): records are cut out of the text and converted by a pool of
 * threads, a batch at a time.  bases hold 0..3 (FASTQ keeps other bytes as (char)-2, as the
 * reference does); offsets[nSeq+1]; names = the record ids. */
typedef struct MgSeqReader MgSeqReader ;
typedef struct { char *bases ; int64_t *offsets ; char **names ; int nSeq ; int64_t total ; int isFastq ; int64_t basesCap ; } MgSeqBatch ;   /* release with mgSeqBatchFree only */
MgSeqReader *mgSeqOpen (const char *filename) ;                        /* 0 if unreadable, empty or not FASTA/FASTQ text */
int  mgSeqNextBatch (MgSeqReader *r, int64_t maxBases, MgSeqBatch *out) ; /* whole records, at least one; 0 at the end */
void mgSeqBatchFree (MgSeqBatch *b) ;
void mgSeqClose (MgSeqReader *r) ;
void mgSeqReleaseBuffers (void) ;	/* the readers keep their two largest buffers for the next file (unmapping and touching gigabytes again costs as much as parsing them); this gives them back -- a no-op while a reader is open; also run when the library is unloaded */
void mgReleaseBuffers (void) ;	/* everything the library caches between calls: the readers' buffers (mgSeqReleaseBuffers), the device buffers and pinned staging of the host-buffer entry points (mgAddSequenceBatch, mgUploadPack: they live on the device the last call ran on and are re-made by themselves when the caller moves to another one), the calling thread's iterator scratch (modRCiterator), the page-locked blocks and device arrays mgQueryFile leaves */
/* Plain FASTA / FASTQ text parsed ON THE DEVICE (the host only moves the bytes: parallel pread into pinned memory, the text as it
 * is across PCIe, record starts / headers / bases found by small kernels per window): mgAddSequenceFile, mgReferenceFastaRead and
 * mgQueryFile take this path by themselves for plain text, for blocked gzip (BGZF) from end to end and for ordinary gzip of at least
 * MODGPU_GZIP_MIN_KB -- both inflated on the device into the same windows; MODGPU_BGZF_HOST=1 / MODGPU_GZIP_HOST=1: by the reader above -- and
 * use the reader above for smaller gzip files, a file that does not end in a newline, a FASTA file whose last line is a header, FASTQ that
 * breaks a rule (from the first record not handed on).  The text of an ordinary gzip file has no known end before its last byte is inflated: such
 * a FASTA file that ends without a newline or in a header line is handed to the reader above at its last record's '>', the records before it added.
 * This entry returns the parser's records as host arrays (bases 0..3 one per byte, offsets[nSeq + 1]; free () both): 0 = done,
 * -1 = error (mgLastError), -2 = not a file the device parser takes as a whole (nothing is returned). */
int  mgTextParseFileDevice (const char *filename, char **bases, int64_t **offsets, int64_t *nSeq) ;
/* test hook: the reader that takes a file up where the device parser hands it over -- from the record that starts at byte startOff of the
 * file's TEXT (a file offset for plain text, the offset in the inflated text for blocked and for ordinary gzip -- the latter has no index: the text
 * before the offset is inflated on the host and dropped), which is line startLine and record startSeq + 1 of the file; 0 for an offset at or past
 * the text's end, for a pipe */
MgSeqReader *mgSeqOpenAt (const char *filename, U64 startOff, U64 startLine, U64 startSeq) ;
/* of the calling thread's last file call (mgAddSequenceFile, mgAddSequenceFile10x, mgReferenceFastaRead, mgQueryFile, mgRefPaintFile,
 * mgTextParseFileDevice ..): which parser took the file -- 0 the host parser from the start, 1 the device parser over plain text, 2 the
 * device parser over blocked gzip inflated on the device, 3 the device parser over ordinary gzip inflated on the device --, windows parsed on the
 * device, text bytes parsed on the device, the text offset handed to the host parser (0: none) */
void mgTextFileDiag (U64 out4[4]) ;
/* the callers' per-file loops: parsing of the next batch overlaps the GPU work on the current one */
int  mgAddSequenceFile (Modset *ms, const char *filename, FILE *out) ;                        /* modutils.c:33-51 */
int  mgReferenceFastaRead (MgReference *ref, const char *filename, bool isAdd, FILE *out) ;   /* modmap.c:93-134 */
/* modutils -x (modutils.c:33-51 with is10x): records are numbered from 1 through the file, and a record with an odd number loses its
 * first 23 bases -- the 10x barcode and UMI -- as the reader delivers them (FASTA: after the non-bases were dropped, so the 23 may span
 * lines).  "total length" counts the untrimmed reads, "total hashes" what the trimmed ones give.  An odd record of fewer than 23 bases
 * becomes an empty read (the reference aborts on it: assert (len >= 0), seqhash.c:156).
 *   mgAddSequenceFile10x     the file loop: plain text is parsed on the device and every batch trimmed there, gzip, a last line without
 *                            its newline and the rest of a FASTQ file that breaks a rule go through the host parser and
 *                            mgAddSequenceBatch10x.  0 / -1 as mgAddSequenceFile, and its line to out.
 *   mgAddSequenceBatch10x    mgAddSequenceBatch for a batch whose first record has number firstOrdinal (1 + the records before it).
 *   mgTrim10xDevice          the trim itself, on a batch in device memory: dPackedOut (mgPackedWords (totalBases) words are enough) and
 *                            dOffOut[nReads + 1] receive the trimmed batch, *totalOut its bases; the call waits for them.  A batch of
 *                            more than (2^32 - 1) / 23 records is refused (MG_ERR_ARG).
 *   mgAdd10xDiag             the calling thread's last mgAddSequenceFile10x: batches trimmed on the device, records with an odd number,
 *                            bases dropped, 1 if the host parser took any part of the file. */
int     mgAddSequenceFile10x (Modset *ms, const char *filename, FILE *out) ;
int64_t mgAddSequenceBatch10x (Modset *ms, const char *bases, const int64_t *readOffsets, int nReads, uint64_t firstOrdinal) ;
MgStatus mgTrim10xDevice (const U32 *dPacked, U64 totalBases, const U64 *dOff, U32 nReads, U64 firstOrdinal,
                          U32 *dPackedOut, U64 *dOffOut, U64 *totalOut, void *stream) ;
void    mgAdd10xDiag (U64 out4[4]) ;
/* modutils -s / -sM (modutils.c:205-219) without the mirror: with a device table the depths are taken where they are -- min (65535,
 * synced depth + pending count) -- by one kernel over the table, against info[] uploaded from the host and copied back to it; the
 * table is left as it was (nothing is folded or synced, no byte of value[] or depth[] moves).  The class is the reference's else-if
 * chain in int arithmetic, whatever the thresholds' order; -s keeps bits 2..7 of info[], -sM only sets bits.  A set without a device
 * table takes the reference's loop over the host arrays.  Neither prints: follow with mgModsetSummaryDevice.  0 / -1 */
int  mgModsetSetCopy (Modset *ms, int copy1min, int copy2min, int copyMmin) ;
int  mgModsetSetCopyM (Modset *ms, int copyMmin) ;
int  mgModsetSetCopyPath (void) ;   /* test hook: the calling thread's last call of the two: 0 = on the device, 1 = the host loop (the set has no device table), -1 = it failed */
/* modsetSummary's bytes (modset.c:130-153) for a set with a device table, without bringing it to the host: the depth histogram
 * (pending counts included) and the four copy tallies are counted on the device and 65540 counters come back.  modsetSummary itself
 * keeps its sync; a set without a device table goes to it.  0 / -1 (nothing is printed then) */
int  mgModsetSummaryDevice (Modset *ms, FILE *f) ;
int  mgQueryFile (MgReference *ref, const char *filename, FILE *out) ;                        /* modmap.c:188-281 */
/* modutils' two commands that read a set already built (the set itself is not changed: not its max, entries or depths; a lookup may
 * bring a device table to the lookup load, as modsetFindBatchDevice does).  The lookups, the depth gathers and the formatting of the
 * text run on the device (mg_report.hip); the host copies the text out and a writer thread puts it to the FILE * in order.  Depths
 * are those after every pending add, counts not yet synced to the host included (the host depth[] receives them as modsetSyncToHost
 * would bring them).  0 = done, -1 = error (mgLastError); without a HIP device both fail (there is no CPU fallback).
 *
 * mgReportDepths: modutils.c:65-77 ("-d"): for i = 1 .. ms->max one line "MH	%llx	%d	%u" (value[i], msCopy (ms, i), depth[i]), then
 * "	%u" per other set, the depth of value[i] there (0 if absent), and "
".  The other sets may come straight from modsetRead: their
 * device tables are made on first use and LEFT RESIDENT (release them with mgModsetDeviceRelease, or modsetDestroy).  A value wider than
 * an other set's 2k bits is answered 0 without a lookup in that set (it holds only values below 4^k). */
int  mgReportDepths (Modset *ms, Modset **others, int nOthers, FILE *f) ;
/* modutils.c:260-273 ("-P") on records already in memory (bases 0..3, offsets[n+1], names[n]): "painting %s length %d\n" per record,
 * then "  %d\t%d\n" (pos, depth) for every modimizer of the record found in ms, in modRCnext order -- also for a record shorter than k
 * or empty (its header alone).  N is base 0 here as everywhere in the library: the reference's -P reads its file through dna2indexConv,
 * which maps N to 0 only after an earlier -a (modutils.c:39; without one its iterator reads past patternRC[]), so compare with
 * `-a ... -P`.  The reference prints to stdout; these write to `out`. */
int  mgRefPaint (Modset *ms, const char *bases, const int64_t *offsets, int nSeq, const char **names, FILE *out) ;
/* the same from a FASTA / FASTQ file: plain text through the device parser, gzip, an unterminated last line or FASTQ that breaks a
 * rule through the host parser, as mgQueryFile.  An unreadable file: -1 with "failed to open ref seq file <name>" (modutils.c:262). */
int  mgRefPaintFile (Modset *ms, const char *filename, FILE *out) ;
/* modutils' text form of a set (modutils.c:169-199): the header line "modset bits B size S k K w W seed SEED", then one line
 * "index<TAB>k-mer letters<TAB>depth<TAB>info" per entry.  Without a HIP device both fail (there is no CPU fallback; mgModsetWriteText
 * above is the host loop, and works on a host-only set).
 *
 * mgModsetWriteTextDevice: modutils.c:191-199 ("-wt") with the lines formatted on the device (mg_report.hip).  Depths are those after
 * every pending add (as mgReportDepths), info[] is the host's.  The set is not changed (a set without a device table gets one, as
 * with mgReportDepths; one that holds a value of 4^k or more -- mgModsetReadText's path 2 -- is refused: write it with
 * mgModsetWriteText).  0 = done, -1 = error (mgLastError). */
int     mgModsetWriteTextDevice (Modset *ms, FILE *f) ;
/* mgModsetReadText: modutils.c:169-190 ("-rt"): creates the Seqhash and the Modset the header names and fills it from the size - 1
 * lines that follow (lines after those are ignored).  0 = error: mgLastError holds the text the reference die()s with ("failed to open
 * text file %s", "failed to read first line of text file %s\n", "bad line %d", and what seqhashCreate / modsetCreate would die() on,
 * checked before they are called).  The caller destroys the set and its hasher.
 *   The file's bytes go to the device as they are and are parsed there (mg_settext.hip) against the grammar -wt writes:
 * "-?[0-9]{1,9}" TAB, a token of 1..32 bytes without white space, TAB, "[0-9]{1,9}" TAB, "[0-9]{1,9}" "\n", the token exactly k bytes
 * long.  c C g G t T are 1 2 3, every other byte 0 (modutils.c:178-184); a k-mer that occurs on several lines keeps its LAST line's
 * depth and info and its FIRST line's place, as the reference's loop leaves it.  A file with any other line is parsed on the host by
 * the reference's own fscanf format (blanks for tabs, empty lines, "+6", several records on a line) and inserted on the device; if a
 * token longer than k gives a value of 4^k or more -- which no device table may hold -- the set is built by the host algorithm and has
 * no device table.  A token longer than 32 bytes overruns a static buffer in the reference (undefined behaviour): here it is
 * "bad line N".
 *   On return ms->max, depth[] and info[] are current on the host; value[] and index[] of a set built on the device reach the host
 * arrays with modsetSyncToHost, as for any set built there (the call has NOT synced them). */
Modset *mgModsetReadText (const char *filename) ;
int     mgModsetReadTextPath (void) ;   /* test hook: what the calling thread's last mgModsetReadText did: 0 = parsed on the device, 1 = parsed on the host and inserted on the device, 2 = built on the host, -1 = it failed before it chose */
int  mgFormatF2 (char *buf64, double x) ;	/* test hook: the "%.2f" of the Q / M lines as the library's parallel formatter writes it (glibc's rounding of the double's exact value, in integer arithmetic; snprintf itself for nan / inf / negative); returns the length */

/* The reference's `composition` program (composition.c:32-121) on the device: a FASTA or FASTQ file's records, their lengths, its bases
 * and qualities.  flags: MG_COMP_BASES (-b), MG_COMP_QUALS (-q), MG_COMP_LENGTHS (-l); -t's rusage lines are not provided.  The program's
 * stdout goes to `out`, its "incomplete sequence record line N" to `err` (either may be 0), the counts into *res (may be 0).  The file's
 * bytes -- plain, or inflated by the host if it is gzip, as the reference reads everything through gzread -- cross to the device in the
 * device text parser's windows (MODGPU_TEXT_WINDOW_KB) and are counted there (mg_composition.hip); there is no host computation of the
 * counts, and without a HIP device the call fails like every batch entry point.  FASTA: a record starts at a '>' that begins a line; of
 * its sequence lines the letters ABCDGHKMNRSTVWY count as their upper case, '-' as itself, every other byte is dropped (seqio.c:49,322).
 * FASTQ: four lines a record, the sequence line counted as it is, qualities as byte - 33.  lenMin follows composition.c:64: an empty record
 * resets it (lengths 5, 0, 100 give 100).
 *   Returns 0, or -1 with mgLastError () and nothing written to `out`:
 *   - FASTQ that breaks a rule, with the reference's words: "no initial @ for FASTQ record line N", "missing + FASTQ line N", "qual not
 *     same length as seq line N";
 *   - a byte the reference would index a table out of bounds with -- 0x80 or above in a FASTA sequence line, or in a FASTQ sequence line
 *     with MG_COMP_BASES; a quality byte below 33 or from 0x80 with MG_COMP_QUALS -- named by its file offset (without the flag that touches
 *     the byte, the file is fine);
 *   - MG_COMP_LENGTHS where lenMin < lenMax and every record is shorter than 4 bases: the reference divides by zero (composition.c:107).
 *     *res is filled all the same;
 *   - a record of 2^31 bases or more; an empty or unreadable file; text whose first byte is neither '>' nor '@' (binary, ONEcode and
 *     BAM input are not read).
 *   A last record the reference drops as unfinished (no final newline, a FASTA file that ends in a header line, a FASTQ file that ends
 * inside a record) is dropped here, too: the message goes to `err`, the records before it are reported, the return is 0. */
#define MG_COMP_BASES 1
#define MG_COMP_QUALS 2
#define MG_COMP_LENGTHS 4
typedef struct {
  int type ;                         /* 1 fasta, 2 fastq */
  U64 nSeq, totLen, lenMin, lenMax ;
  U64 base[256], qual[256] ;         /* zero where the flag was not set */
  U32 nBins ; int *binCount ; U64 *binSum ;   /* -l: malloc'ed, [nBins], bin isqrt (100 len); 0 without the flag */
} MgComposition ;
int  mgCompositionFile (const char *filename, int flags, FILE *out, FILE *err, MgComposition *res) ;
int  mgCompositionText (const char *text, U64 n, int flags, FILE *out, FILE *err, MgComposition *res) ;   /* the same on text in host memory: the file's bytes, already inflated */
void mgCompositionFree (MgComposition *res) ;   /* the arrays; res itself is the caller's */
void mgCompositionDiag (U64 out4[4]) ;           /* of the calling thread's last call: windows, tiles of 4 KiB, records that crossed a window edge, kernel launches */

/* The reference's `seqconvert -fa|-fq` (seqconvert.c) and `seqhoco` (seqhoco.c) on the device: a FASTA or FASTQ file rewritten as FASTA or
 * FASTQ.  The text -- plain, or inflated by the host if it is gzip -- crosses to the device in the device text parser's windows, every byte
 * is classified, compacted and re-emitted there (mg_seqconvert.hip), and the host writes what comes back; it computes nothing per byte.
 * The text goes through twice: once to judge it (nothing is written before the whole of it is known to be acceptable, and the walk finds
 * where an unfinished last record or seqhoco's stop begins), once to write it.
 *   Header line (seqio.c:303-313): the id ends at the first white-space byte; if that is not the newline, the rest of the line is the
 * description.  Written: '>' or '@', the id and -- only if the description is not empty -- one space and the description ("r1\tx" becomes
 * "r1 x", "r2 " becomes "r2", a CRLF header loses its '\r' where that is the separator).
 *   FASTA in: a record starts at a '>' that begins a line; of its sequence lines the letters ABCDGHKMNRSTVWY are written in upper case and
 * '-' as itself, every other byte is dropped; one line a record.  FASTQ in: four lines a record, sequence and quality lines written as they
 * are, the '+' line as "+".  FASTQ out of FASTA: the quality line is '!' for every base.  An empty record is written with empty lines.
 *   MG_SEQ_HOCO: FASTA in keeps ACGTNacgtn only; within a record a kept byte is written iff it is the first or differs under toupper from
 * the kept byte before it ("aAaA" -> "a"); no descriptions; the output is FASTA and ends before the first record whose kept length is 0
 * (seqhoco.c:26).  The byte from beyond the sequence that the program appends to every line (seqhoco.c:29-30) is not written.
 *   outName: "-" stdout, "-z" stdout gzipped, a name ending in .gz a gzip file (mgGzipOpenWrite).  Without MG_SEQ_FASTA / MG_SEQ_FASTQ /
 * MG_SEQ_HOCO the type is the name's .fa / .fq suffix (before .gz), as in seqio.c:426-428.  The program's stderr chatter is not provided;
 * its counters are in *res (may be 0).
 *   Returns 0, or -1 with mgLastError (), nothing written to `out` and the output file removed -- whatever the failure, and also a file of
 * that name that was there before the call and that the call never opened (the program would have truncated it when it opened its output):
 *   - FASTQ that breaks a rule, in the reference's words (see mgCompositionFile);
 *   - a byte from 0x80 in a FASTA sequence line; with MG_SEQ_HOCO and FASTQ in, a sequence byte outside ACGTNacgtn (the program indexes a
 *     table out of bounds with either); a NUL byte in a header line (the program's strlen would cut the name there) -- named by file offset;
 *   - a record of 2^31 bases or more; an empty or unreadable file; text that starts with neither '>' nor '@';
 *   - both type flags; MG_SEQ_HOCO with MG_SEQ_FASTQ; no type from flags or name (the program would write its binary format, which its
 *     own reader does not read back: seqio.c:573-581).
 *   An unfinished last record is dropped, "incomplete sequence record line N" goes to `err`, the return is 0 (see mgCompositionFile). */
#define MG_SEQ_FASTA 1
#define MG_SEQ_FASTQ 2
#define MG_SEQ_HOCO 4
typedef struct {
  int inType, outType ;                       /* 1 fasta, 2 fastq */
  U64 nSeq, totSeqLen, maxSeqLen ;            /* of what was WRITTEN: seqconvert's "written N sequences ... total length ... max length" */
  U64 totIdLen, totDescLen, maxIdLen, maxDescLen ;
  U64 nSeqIn, totSeqLenIn ;                   /* complete records read / their bases after the input filter (differs under HOCO) */
} MgSeqConvert ;
int  mgSeqConvertFile (const char *inName, const char *outName, int flags, FILE *err, MgSeqConvert *res) ;
int  mgSeqConvertText (const char *text, U64 n, int flags, FILE *out, FILE *err, MgSeqConvert *res) ;   /* input already inflated, output to `out` */
void mgSeqConvertDiag (U64 out4[4]) ;   /* calling thread's last call: windows, 4 KiB tiles, records that crossed a window edge, kernel launches */

/* Blocked gzip (BGZF: bgzip, htslib) inflated on the device.  A BGZF file is a row of gzip members of at most 64 KiB, compressed and not,
 * each an independent raw-deflate stream with its own CRC-32 and length: one wave inflates one member (mg_inflate.hip).
 *   mgInflateMembersDevice: n members of the device buffer dComp into the device buffer dOut.  members[] (host) names each one's deflate
 * payload -- offset and length WITHOUT the gzip header and trailer -- its place in dOut, and the CRC-32 and length its trailer states.
 * No slack is asked of either buffer: the decoder reads and writes single bytes inside [cOff, cOff + cLen) and [uOff, uOff + uLen) only.
 * A member whose cLen or uLen exceeds 65536 or whose ranges leave compBytes / outBytes is refused with MG_ERR_ARG before anything is
 * launched.  status[i] (host, may be 0): 0 ok, 1 input exhausted, 2 bad block type, 3 stored LEN/NLEN mismatch, 4 bad code lengths,
 * 5 invalid symbol, 6 distance beyond the member's start, 7 output longer or shorter than stated, 8 CRC mismatch; *nBad the members whose
 * status is not 0 (a bad member does not stop the others; what its range of dOut holds is undefined, nothing outside it is written).
 * Returns when the launch is over (it waits for `stream`).
 *   mgInflateMemberHost: the same decoder compiled for the host, one member on the calling thread -- a test hook, as mgIterScanHost is.
 * stats8 (may be 0): deflate blocks stored / fixed / dynamic, longest literal/length code, longest distance, longest match, longest
 * distance code, literal/length symbols.  Returns 0 (the verdict is *status), -1 on a null argument.
 *   mgBgzfInflateFile: `bgzip -d`: the file's text to outName ("-": stdout).  0, or -1 with mgLastError () and no output file left;
 * -2: not a BGZF file from its first byte to its last (nothing is written).
 *   mgCompositionFile and mgSeqConvertFile take this path for a file that is BGZF from end to end (MODGPU_BGZF_HOST=1: never). */
typedef struct { U64 cOff; U64 uOff; U32 cLen; U32 uLen; U32 crc; U32 pad; } MgGzMember;   /* deflate payload: offset and length without header and trailer */
MgStatus mgInflateMembersDevice (const U8 *dComp, U64 compBytes, const MgGzMember *members /* host */, U32 n,
                                 U8 *dOut, U64 outBytes, U32 *status /* host, [n]; may be 0 */, U32 *nBad, void *stream) ;
void     mgInflateDiag (U64 out4[4]) ;   /* calling thread's last call: members inflated on the device, compressed bytes uploaded, text bytes produced, kernel launches */
int      mgInflateMemberHost (const U8 *comp, U32 cLen, U8 *out, U32 uLen, U32 crc, U32 *status, U64 stats8[8]) ;
int      mgBgzfInflateFile (const char *inName, const char *outName /* "-": stdout */, FILE *err) ;

/* Ordinary gzip (gzip, pigz, zlib: one member or several, no block table) inflated on the device (mg_gunzip.hip over mg_gunzip_core.h): block starts
 * are found by testing bit offsets, chunks are decoded speculatively into 16-bit symbols, the chain of chunks is confirmed, the 32 KiB window is carried
 * from chunk to chunk and the symbols are resolved into bytes; every member's CRC-32 and ISIZE are checked.
 *   mgGzipInflateFile: `gzip -dc`: the file's text to outName ("-": stdout).  0, or -1 with mgLastError () and no output file left; -2: not a gzip
 * file (or a first member with a 'BC' field, or more than the device keeps: nothing is written).
 *   mgGunzipHost: the same pipeline compiled for the host, on the calling thread -- a test hook and the device's yardstick.  comp[0 .. n) is the gzip
 * file, chunkBytes the compressed bytes per chunk (4096 at least), batchChunks the chunks per batch, symbolsPerChunk the room a chunk's symbols get
 * before the retry.  *status: 0, the codes of mgInflateMembersDevice, 9 = a single chunk needs more than 2^28 symbols, 10 = not a gzip header where one
 * must be (bytes behind a trailer included).  Nothing outside out[0 .. cap) is written; text longer than cap is status 7.  Returns 0 (the verdict is
 * *status), -1 on a null argument or no memory.
 *   mgGunzipDiag: the calling thread's last mgGzipInflateFile / mgCompositionFile / mgSeqConvertFile: chunks speculated, confirmed, discarded after a
 * chain break, folded (no candidate), batches, members, capacity retries, kernel launches -- all 0 if the file did not take this path.  diag8 of
 * mgGunzipHost counts the same.
 *   mgCompositionFile and mgSeqConvertFile take this path for an ordinary gzip file of at least MODGPU_GZIP_MIN_KB (MODGPU_GZIP_HOST=1: never); they
 * walk the text twice and keep the compressed file on the device (8 GiB and a quarter of the free memory at the most).
 *   mgAddSequenceFile, mgAddSequenceFile10x, mgReferenceFastaRead and mgQueryFile take it from the same size up and walk once: the compressed bytes pass
 * through a bounded range on the device, every byte uploaded once, whatever the file's size.  mgGzipSrcDiag: of the calling thread's last such call the
 * compressed bytes uploaded, the range's refills, the most compressed bytes resident at once, and the bound on them -- twice (chunks a batch + 1) *
 * chunk bytes + one upload piece; a single deflate block longer than that makes the range grow past it. */
void     mgGzipSrcDiag (U64 out4[4]) ;
int      mgGzipInflateFile (const char *inName, const char *outName /* "-": stdout */, FILE *err) ;
int      mgGunzipHost (const U8 *comp, U64 n, U32 chunkBytes, U32 batchChunks, U32 symbolsPerChunk, U8 *out, U64 cap, U64 *outLen, U32 *status, U64 diag8[8]) ;
void     mgGunzipDiag (U64 out8[8]) ;

/* Blocked gzip (BGZF) deflated on the device: the writer's half.  Text is cut into blocks of at most 65280 bytes (bgzip's), each block becomes
 * one complete BGZF member of at most 65536 bytes -- the 18-byte header with the 'BC' field, ONE raw-deflate block, CRC-32 and length -- and
 * one workgroup deflates one block (mg_deflate.hip over mg_deflate_core.h): LZ77 with a one-candidate hash of the next 4 bytes, then the
 * cheapest of a stored block, a dynamic-Huffman block of literals only and a dynamic-Huffman block with the matches, by their exact bit
 * costs.  A member is a pure function of its block's bytes: the host compile of the core writes the same bytes as the kernel.
 *   mgDeflateBlocksDevice: blocks[i] (host) names n ranges [uOff, uOff + uLen) of the device buffer dText; their members are written to
 * dOut packed, in order, from dOut[0]; memberOff[i] (host, n + 1 entries) is where member i begins, memberOff[n] the bytes written, and
 * nothing beyond that is written.  Refused with MG_ERR_ARG before anything is launched: uLen > 65280, a range that leaves textBytes,
 * outBytes < 65536 * n.  Returns when `stream` is idle.
 *   mgDeflateBlockHost: the same encoder compiled for the host, one block on the calling thread into out[0 .. 65536) -- a test hook.
 * stats8 (may be 0): the kind written (0 stored, 1 literals only, 2 with matches), literals, matches, longest match, longest distance,
 * longest literal/length code, longest distance code, payload bits.  Returns 0, -1 on a null argument or uLen > 65280.
 *   mgBgzfDeflateFile: `bgzip`: any regular file to outName as BGZF with bgzip's 28-byte end-of-file member (an empty file gives that
 * member alone).  0, or -1 with mgLastError () and no output file left.
 *   mgSeqConvertFileBgzf: mgSeqConvertFile in every respect -- flags, the type from a .fa / .fq suffix (here before an optional .gz or
 * .bgz), refusals and their words, *res, no file after a refusal, BGZF input inflated on the device -- but the second walk's output never
 * crosses the link as text: it is deflated on the device and written as BGZF whatever the name's suffix.
 *   MODGPU_BGZF_BLOCK: text bytes per member, 1 .. 65280 (default 65280; the tests cross block boundaries with small files). */
typedef struct { U64 uOff; U32 uLen; U32 pad; } MgGzBlock;
MgStatus mgDeflateBlocksDevice (const U8 *dText, U64 textBytes, const MgGzBlock *blocks /* host */, U32 n,
                                U8 *dOut, U64 outBytes, U64 *memberOff /* host, [n + 1] */, void *stream) ;
int      mgDeflateBlockHost (const U8 *text, U32 uLen, U8 *out /* 65536 */, U32 *outLen, U64 stats8[8]) ;
void     mgDeflateDiag (U64 out4[4]) ;   /* calling thread's last call: blocks deflated on the device, text bytes in, file bytes out, kernel launches */
int      mgBgzfDeflateFile (const char *inName, const char *outName, FILE *err) ;
int      mgSeqConvertFileBgzf (const char *inName, const char *outName, int flags, FILE *err, MgSeqConvert *res) ;

/* Deterministic synthetic reads generated directly in HBM (not from the reference):
 *   mgSynthGenome: nBases iid-uniform bases, base g = splitmix64(seed ^ g*0x9E3779B97F4A7C15) >> 62
 *   mgSynthReads : read r = genome[start[r], start[r]+len[r]) reverse-complemented when
 *                  strand[r] != 0, each base substituted with probability errRate (a counter-based
 *                  hash of (seed, global base ordinal) decides), written 2-bit packed. */
MgStatus mgSynthGenome (U32 *dPacked, U64 nBases, U64 seed, void *stream) ;
MgStatus mgSynthReads (const U32 *dGenomePacked, U64 genomeBases,
                       const U64 *dReadStart, const U64 *dReadOffsets, const U8 *dStrand, U32 nReads,
                       U64 totalBases, double errRate, U64 seed, U32 *dPackedOut, void *stream) ;

/* Per-kernel timing with HIP events on the launch stream (for bench.py's roofline object).
 * While enabled, every kernel launch of the library is bracketed by an event pair; mgProfileGet
 * returns, per kernel id in [0, mgProfileKernels()), its name, summed duration and launch count
 * since the last mgProfileReset (it synchronises the device to read the events). */
void     mgProfileEnable (int on) ;
void     mgProfileOnly (int kernelId) ;     /* >= 0: only that kernel is bracketed (an event pair costs a few microseconds of stream time per launch); -1: all */
void     mgProfileReset (void) ;
int      mgProfileKernels (void) ;
MgStatus mgProfileGet (int id, const char **name, double *totalMs, U64 *launches) ;

#ifdef __cplusplus
}
#endif
#endif /* MODGPU_H */
