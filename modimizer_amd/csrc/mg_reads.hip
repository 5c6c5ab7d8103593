/* mg_reads.hip — a device-resident batch of reads against a Modset: the scan into the set's scratch arena with a capacity that is first
 * a guess, then the set's build (mgAddReadsDevice), the seed lists with lookups or inserts (mgQueryReadsDevice, mgInsertReadsDevice,
 * mgSeedsOfBatch), and the two-slot pipeline that scans the next query batch beside the lookups of this one
 * (mgQueryReadsDeviceAsync / mgQueryReadsDeviceWait).
 */
#include "mg_api_int.h"

struct MgScanBufs { U64 *kmer; U32 *posF; U32 *rid; void *work; U64 *count; U64 cap; MgHistReq counted;
                    MgSegSrc seg; bool lazy; void *findScratch, *findScratch2; };      /* lazy: kmer[] has not been written, the modimizers are in seg */

/* outPosF / outRid (with room for outCap entries): the caller's own arrays; when they are large enough for the scan's
 * capacity the compaction writes pos / read straight into them (a device-to-device copy of 1.2 GB per 10 Gbp batch
 * took longer than the scan itself) */
struct MgScanReq { const Seqhash *sh; const U32 *dPacked; U64 totalBases; const U64 *dReadOffsets; U32 nReads; bool wantPos; size_t extraPerSurvivor;
                   U32 *outPosF, *outRid; U64 outCap; bool lazy; };
static inline U64 *mgCountPin (MgDev *d, int slot) { return d->hPin + 8 + 8 * slot; }

/* launch: buffers out of the slot's arena for `cap` modimizers, the scan, its counters on their way to the slot's pinned words.  No
   wait: mgScanFinish does that */
static MgStatus mgScanStart (MgDev *d, int slot, const MgScanReq &q, U64 cap, MgScanBufs *b, hipStream_t st)
{
  b->lazy = false; b->seg.nSegs = 0; b->seg.segKmer = 0; b->findScratch = 0; b->findScratch2 = 0;
  MgArena &ar = mgArenaOf (d, slot);
  /* a lookup batch whose k-mers stay in the segments may take the partitioned path (mgTableFindPartitioned): it needs the first digit's counts */
  const long fp = mgKnobs ()->findPath;
  const bool lookupHist = q.lazy && q.wantPos && !q.extraPerSurvivor && d->t.slots && fp != 'd'
                          && (fp == 'p' || fp == '2' || (cap >= ((U64) 1 << 24) && d->t.nSlots >= ((U64) 1 << 24) && d->t.log2NB > 9));
  const bool lookup2 = lookupHist && fp != 'p';
  MgHashParams p = mgMakeParams (q.sh);
  const size_t perS = 8 + (q.wantPos ? 8 : 0) + q.extraPerSurvivor;
  const size_t need = mgAl256 (cap * perS) + 4 * 4096 + 512 * MG_HIST_STRIDE * 4 + mgAl256 (mgScanWorkBytes (q.totalBases, q.nReads, cap))
                      + (q.extraPerSurvivor ? mgTableAddScratchBytes (&d->t, cap < MG_ADD_CHUNK ? cap : MG_ADD_CHUNK) + 8192 : 0) + 8 * 256
                      + (lookupHist ? mgTableFindPartScratchBytes (cap) + 8192 : 0) + (lookup2 ? mgTableFindPart2ScratchBytes (cap) + 8192 : 0);
  MgStatus s = mgArenaOpen (d, slot, need); if (s) return s;      /* (a value writer still reading that arena is waited for: the callers pick the other one where they can) */
  b->cap = cap;
  b->kmer = (U64 *) ar.take (cap * 8);
  const bool direct = q.wantPos && q.outPosF && q.outRid && q.outCap >= cap;
  b->posF = !q.wantPos ? 0 : (direct ? q.outPosF : (U32 *) ar.take (cap * 4));
  b->rid = !q.wantPos ? 0 : (direct ? q.outRid : (U32 *) ar.take (cap * 4));
  b->work = ar.take (mgScanWorkBytes (q.totalBases, q.nReads, cap));
  b->count = (U64 *) ar.take (8 * MG_COUNT_WORDS);
  b->counted.log2NB = 0; b->counted.kbits = 64; b->counted.binCount = 0; b->counted.hiB = 0;
  if (q.extraPerSurvivor || lookupHist)              /* the survivors go into the modset, or through the partitioned lookup: have the scan count the first partition digit */
    { b->counted.binCount = (U32 *) ar.take (512 * MG_HIST_STRIDE * sizeof (U32));
      b->counted.log2NB = d->t.log2NB; b->counted.kbits = d->t.kbits;
      if (lookupHist) b->counted.hiB = mgTableFindDigitBits (&d->t);
    }
  b->findScratch = lookupHist ? ar.take (mgTableFindPartScratchBytes (cap)) : 0;
  b->findScratch2 = lookup2 ? ar.take (mgTableFindPart2ScratchBytes (cap)) : 0;
  const bool lz = q.lazy && (q.wantPos ? q.extraPerSurvivor == 0 : b->counted.binCount != 0);   /* a build needs the digit counts; a pure lookup just the segments */
  if ((s = mgLaunchScan (p, q.dPacked, q.totalBases, q.dReadOffsets, q.nReads, b->kmer, b->posF, b->rid, cap, b->count, b->work, st,
                         b->counted.binCount ? &b->counted : 0, lz ? &b->seg : 0))) return s;
  b->lazy = lz;
  MG_HIP (hipMemcpyAsync (mgCountPin (d, slot), b->count, MG_COUNT_WORDS * sizeof (U64), hipMemcpyDeviceToHost, st));
  return MG_OK;
}
/* wait for the scan; *nOut = its modimizers, or *retryCap != 0: the capacity was too small, start again with that one */
static MgStatus mgScanFinish (MgDev *d, int slot, const MgScanBufs *b, U64 *nOut, U64 *retryCap, hipStream_t st, hipEvent_t done = 0)
{
  if (done) MG_HIP (hipEventSynchronize (done));           /* (this scan alone: the stream may hold the next batch's scan behind it) */
  else MG_HIP (hipStreamSynchronize (st));
  *retryCap = mgScanRetryCap (mgCountPin (d, slot), b->cap, nOut);
  return MG_OK;
}

/* the scan of q into the slot's arena on st, its capacity a guess at first: at most three scans, each after the first with the capacity the
   one before asked for.  started: the first of them is running already, into b -- for cap modimizers, with this event recorded behind it */
static MgStatus mgScanRounds (MgDev *d, int slot, const MgScanReq &q, U64 cap, MgScanBufs *b, U64 *nOut, hipStream_t st, hipEvent_t started = 0)
{
  for (int round = 0 ; round < 3 ; ++round)
    { MgStatus s;
      const bool running = started && !round;
      if (!running && (s = mgScanStart (d, slot, q, cap, b, st))) return s;
      if ((s = mgScanFinish (d, slot, b, nOut, &cap, st, running ? started : 0))) return s;
      if (!cap) return MG_OK;
    }
  mgSetError ("scan capacity could not be established");
  return MG_ERR_CAPACITY;
}

static MgStatus mgScanIntoArena (MgDev *d, const Seqhash *sh, const U32 *dPacked, U64 totalBases,
                                 const U64 *dReadOffsets, U32 nReads, bool wantPos, size_t extraPerSurvivor,
                                 MgScanBufs *b, U64 *nOut, hipStream_t st,
                                 U32 *outPosF = 0, U32 *outRid = 0, U64 outCap = 0, bool lazy = false, int slot = 0)
{
  MgStatus s = mgDevRefuseInFlight (d); if (s) return s;
  MgScanReq q = { sh, dPacked, totalBases, dReadOffsets, nReads, wantPos, extraPerSurvivor, outPosF, outRid, outCap, lazy };
  if (extraPerSurvivor)
    { /* size the table now for the expected number of modimizers (N/d): the insert would do it anyway once the
         count is known, and with the geometry fixed the scan (or, for 2k < 24, the compaction kernel) can count for the first partition pass */
      U64 expect = totalBases / (U64) (sh->w > 0 ? sh->w : 1) + 1;
      if (expect > MG_ADD_CHUNK) expect = MG_ADD_CHUNK;
      if ((s = mgTableEnsure (&d->t, expect, st))) return s;
    }
  return mgScanRounds (d, slot, q, mgSurvivorGuess (sh, totalBases), b, nOut, st);
}

extern "C" MgStatus mgAddReadsDevice (Modset *ms, const U32 *dPacked, U64 totalBases,
                                      const U64 *dReadOffsets, U32 nReads, U64 *nHash, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  MgDev *d; MgStatus s = mgDevGet (ms, &d, st); if (s) return s;
  if (nHash) *nHash = 0;
  if (!totalBases || !nReads) return MG_OK;
  MgScanBufs b; U64 n = 0;
  d->t.loadPct = 75;                                   /* built and counted: see MgTable.loadPct */
  /* pos / isF / read are not needed by addSequence (modutils.c:24 passes 0 for isF and ignores pos) */
  /* the dense k-mer array is only made if the insert turns out to need it (a small batch, the table regrown): a large
     batch's first partition pass and index assignment read the scan's segments */
  /* the value writer of the add before this one may still be reading its batch out of one arena: this batch goes into the other, and the writer
     runs beside this scan (mgTableAdd).  The arenas take turns whether or not that writer has finished -- no event is asked -- so which add pays
     for the second arena's allocation does not depend on the host's timing; the writer that last read the arena taken here, two adds ago, is
     waited for (mgArenaOpen) and has long finished.  No query ticket holds an arena here: mgScanIntoArena refuses the call while one is out */
  int slot = d->valuePending[d->valueLast] ? d->valueLast ^ 1 : 0;
  if (d->valuePending[slot ^ 1] && mgArenaOf (d, slot).bytes < mgArenaOf (d, slot ^ 1).used)
    { /* the arena whose turn it is was never made as large as the other (mgArenaTwin found no room): once more, and where the device still has none
         this add waits for the pending writer and takes that one's arena, as every add did when a set had one */
      if ((s = mgValueSettle (d, 0, MG_SETTLE_HOST, slot))) return s;
      if (!mgArenaOf (d, slot).tryReserve (mgArenaOf (d, slot ^ 1).used)) slot ^= 1;
    }
  if ((s = mgScanIntoArena (d, ms->hasher, dPacked, totalBases, dReadOffsets, nReads, false, 4, &b, &n, st, 0, 0, 0, true, slot))) return s;
  if (nHash) *nHash = n;
  if (!n) return MG_OK;
  if (b.lazy)
    { const U64 chunk = n < MG_ADD_CHUNK ? n : MG_ADD_CHUNK;
      if ((s = mgTableEnsure (&d->t, chunk, st))) return s;
      if (n <= MG_ADD_CHUNK && mgTableAddTakesSegments (&d->t, n, &b.counted))
        { s = mgAddBatch (ms, d, 0, n, 0, 1, slot, st, &b.counted, &b.seg, true);
          if (!s && d->valuePending[slot]) mgArenaTwin (d, slot);
          return s;
        }
      if ((s = mgLaunchSegCompact (b.seg, b.kmer, b.cap, b.count, st))) return s;
    }
  s = mgAddBatch (ms, d, b.kmer, n, 0, 1, slot, st, &b.counted, 0, true);
  if (!s && d->valuePending[slot]) mgArenaTwin (d, slot);
  return s;
}

/* the seeds of a scanned batch of n modimizers into the caller's arrays of `capacity` entries: their index[] -- ms given: inserted without
   depth (modmap.c:109), else lookups only (modmap.c:202), by the path the scan prepared for --, pos / read copied where the scan did not
   write them there itself, and the stream waited for */
static MgStatus mgSeedsOfScanned (Modset *ms, MgDev *d, MgScanBufs &b, U64 n, U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity, hipStream_t st)
{
  if (n > capacity)
    { mgSetError ("%llu seeds exceed the caller's capacity %llu", (unsigned long long) n, (unsigned long long) capacity); return MG_ERR_CAPACITY; }
  MgStatus s;
  if (ms) s = mgAddBatch (ms, d, b.kmer, n, dSeedIndex, 0, 0, st, &b.counted);
  else if (b.lazy && b.findScratch && mgTableFindTakesPartition (&d->t, n, &b.counted))
    s = mgTableFindPartitioned (&d->t, b.seg, n, &b.counted, dSeedIndex, b.kmer, b.findScratch, st, b.findScratch2);     /* (b.kmer: the dense array a lazy scan leaves unused) */
  else s = b.lazy ? mgTableFindSegments (&d->t, b.seg, n, dSeedIndex, st) : mgTableFind (&d->t, b.kmer, n, dSeedIndex, st);
  if (s) return s;
  if (dSeedPosF && b.posF != dSeedPosF) MG_HIP (hipMemcpyAsync (dSeedPosF, b.posF, n * 4, hipMemcpyDeviceToDevice, st));
  if (dSeedRead && b.rid != dSeedRead) MG_HIP (hipMemcpyAsync (dSeedRead, b.rid, n * 4, hipMemcpyDeviceToDevice, st));
  MG_HIP (hipStreamSynchronize (st));
  return MG_OK;
}

/* mode 0: lookup only (modmap.c:202); mode 1: insert without depth (modmap.c:109).  scanWith (0: the set's own hasher) scans the batch: it has the set's k, the width of the table's keys */
static MgStatus mgSeedReads (Modset *ms, const Seqhash *scanWith, int mode, const U32 *dPacked, U64 totalBases,
                             const U64 *dReadOffsets, U32 nReads,
                             U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity,
                             U64 *nSeeds, hipStream_t st)
{
  MgDev *d; MgStatus s = mgDevGet (ms, &d, st); if (s) return s;
  if (nSeeds) *nSeeds = 0;
  if (!scanWith) scanWith = ms->hasher;
  if ((s = mgCheckHasher (scanWith))) return s;
  if (scanWith->k != ms->hasher->k) { mgSetError ("a batch scanned with k %d cannot be looked up in a set of k %d", scanWith->k, ms->hasher->k); return MG_ERR_ARG; }
  if (!totalBases || !nReads) return MG_OK;
  MgScanBufs b; U64 n = 0;
  d->t.loadPct = MG_LOOKUP_LOAD_PCT;                                   /* lookups follow (or are this call): see MgTable.loadPct */
  if (mode == 0 && d->t.slots && (s = mgTableEnsure (&d->t, 0, st))) return s;
  const int timing = mgKnobs ()->seedTiming == 1;   /* dev */
  struct timespec q0, q1, q2; if (timing) clock_gettime (CLOCK_MONOTONIC, &q0);
  /* lookups read the k-mers from the scan's segments (no dense copy of them); pos / read are compacted as before */
  if ((s = mgScanIntoArena (d, scanWith, dPacked, totalBases, dReadOffsets, nReads, true, mode ? 4 : 0, &b, &n, st,
                            dSeedPosF, dSeedRead, capacity, mode == 0))) return s;
  if (timing) clock_gettime (CLOCK_MONOTONIC, &q1);
  if (nSeeds) *nSeeds = n;
  if ((s = mgSeedsOfScanned (mode ? ms : 0, d, b, n, dSeedIndex, dSeedPosF, dSeedRead, capacity, st))) return s;
  if (timing)
    { clock_gettime (CLOCK_MONOTONIC, &q2);
      fprintf (stderr, "mgSeedReads: scan+count %.2f ms, lookup+sync %.2f ms\n", (q1.tv_sec - q0.tv_sec) * 1e3 + (q1.tv_nsec - q0.tv_nsec) * 1e-6,
               (q2.tv_sec - q1.tv_sec) * 1e3 + (q2.tv_nsec - q1.tv_nsec) * 1e-6);
    }
  return MG_OK;
}

extern "C" MgStatus mgQueryReadsDevice (Modset *ms, const U32 *dPacked, U64 totalBases,
                                        const U64 *dReadOffsets, U32 nReads,
                                        U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity,
                                        U64 *nSeeds, void *stream)
{ return mgSeedReads (ms, 0, 0, dPacked, totalBases, dReadOffsets, nReads, dSeedIndex, dSeedPosF, dSeedRead, capacity, nSeeds, (hipStream_t) stream); }

extern "C" MgStatus mgInsertReadsDevice (Modset *ms, const U32 *dPacked, U64 totalBases,
                                         const U64 *dReadOffsets, U32 nReads,
                                         U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity,
                                         U64 *nSeeds, void *stream)
{ return mgSeedReads (ms, 0, 1, dPacked, totalBases, dReadOffsets, nReads, dSeedIndex, dSeedPosF, dSeedRead, capacity, nSeeds, (hipStream_t) stream); }

/* the seed list of a batch in arrays that this call sizes: the contract is at the declaration (mg_internal.h) */
extern "C" void mgSeedBufsFree (MgSeedBufs *bufs)
{
  (void) hipFree (bufs->ix); (void) hipFree (bufs->posF); (void) hipFree (bufs->rid);
  bufs->ix = bufs->posF = bufs->rid = 0; bufs->cap = 0;
}
static MgStatus mgSeedBufsReserve (MgSeedBufs *bufs, U64 need)
{
  if (bufs->cap >= need) return MG_OK;
  mgSeedBufsFree (bufs);
  const U64 room = need + need * (U64) bufs->sparePct / 100 + 1;
  U32 **arr[3] = { &bufs->ix, &bufs->posF, &bufs->rid };
  for (int j = 0 ; j < 3 ; ++j)
    { const hipError_t e = hipMalloc ((void **) arr[j], room * sizeof (U32));
      if (e != hipSuccess) { *arr[j] = 0; mgSeedBufsFree (bufs); return mgHipFail (e, "a batch's seed arrays"); }
    }
  bufs->cap = room; return MG_OK;
}
extern "C" MgStatus mgSeedsOfBatch (Modset *ms, const Seqhash *scanWith, int insert, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                    U64 guess, MgSeedBufs *bufs, U64 *nSeeds, void *stream)
{
  const bool empty = !totalBases || !nReads;                 /* (the inner call still runs: it validates, and brings the set's device table up) */
  U64 offer = empty ? 0 : (guess < totalBases + 1 ? guess : totalBases + 1);
  *nSeeds = 0;
  for (int attempt = 0 ; ; ++attempt)
    { MgStatus s = mgSeedBufsReserve (bufs, offer); if (s) return s;
      s = mgSeedReads (ms, scanWith, insert ? 1 : 0, dPacked, totalBases, dReadOffsets, nReads, bufs->ix, bufs->posF, bufs->rid, offer, nSeeds, (hipStream_t) stream);
      if (s != MG_ERR_CAPACITY || attempt || *nSeeds <= offer) return s;
      offer = *nSeeds;
    }
}

/* The lookup loop of queryProcess (modmap.c:197-206) for batches that follow one another, in two halves: Async starts the batch's SCAN
 * on a stream of the library's own, into the other of two scratch arenas, and returns; Wait runs its LOOKUPS on the caller's stream and
 * returns when the seeds are complete.  Called as  Async (0); for i: Async (i + 1); Wait (i)  the scan of batch i + 1 -- bound by
 * instruction issue -- runs beside the lookups of batch i -- bound by memory requests (profiles/r03_corun_matrix.txt: 7 - 8 % on the
 * pair).  At most two batches in flight, waited for in the order they were started; each needs its own output arrays; until the last
 * ticket is waited for, the modset takes no other batch call. */
struct MgQueryTicket { Modset *ms; MgDev *d; int slot; MgScanReq q; MgScanBufs b; U32 *dSeedIndex, *dSeedPosF, *dSeedRead; U64 capacity; };

extern "C" MgStatus mgQueryReadsDeviceAsync (Modset *ms, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads,
                                             U32 *dSeedIndex, U32 *dSeedPosF, U32 *dSeedRead, U64 capacity, void **ticket, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  if (!ticket) { mgSetError ("mgQueryReadsDeviceAsync: null ticket"); return MG_ERR_ARG; }
  *ticket = 0;
  MgDev *d; MgStatus s = mgDevGet (ms, &d, st); if (s) return s;
  if (d->ticketsOut >= 2) { mgSetError ("two query batches are in flight already"); return MG_ERR_ARG; }
  d->t.loadPct = MG_LOOKUP_LOAD_PCT;
  if (d->t.slots && !d->ticketsOut && (s = mgTableEnsure (&d->t, 0, st))) return s;      /* (with a batch in flight the table has its lookup shape already) */
  if (!d->side)
    { /* lowest priority: the lookups are a chain of short kernels that should not queue behind the scan's workgroups; the scan fills what they leave */
      int lo = 0, hi = 0; (void) hipDeviceGetStreamPriorityRange (&lo, &hi);
      MG_HIP (hipStreamCreateWithPriority (&d->side, hipStreamNonBlocking, lo));      /* (default priority instead: no difference measured, DESIGN_EXPERIMENTS §J) */
      for (int i = 0 ; i < 2 ; ++i) MG_HIP (hipEventCreateWithFlags (&d->scanned[i], hipEventDisableTiming));
      MG_HIP (hipEventCreateWithFlags (&d->inputReady, hipEventDisableTiming));
    }
  int slot = d->slotBusy[d->nextSlot] ? d->nextSlot ^ 1 : d->nextSlot;
  if (d->valuePending[slot] && !d->slotBusy[slot ^ 1] && !d->valuePending[slot ^ 1]) slot ^= 1;      /* an arena a value writer may still read counts as busy (else mgScanStart waits for the writer) */
  MgQueryTicket *t = new MgQueryTicket ();
  t->ms = ms; t->d = d; t->slot = slot; t->dSeedIndex = dSeedIndex; t->dSeedPosF = dSeedPosF; t->dSeedRead = dSeedRead; t->capacity = capacity;
  t->q = MgScanReq { ms->hasher, dPacked, totalBases, dReadOffsets, nReads, true, 0, dSeedPosF, dSeedRead, capacity, true };
  t->b = MgScanBufs (); t->b.cap = 0;
  if (totalBases && nReads)
    { /* the batch (and a table that has just been reshaped) is ready when the caller's stream gets here: the scan's stream waits for that */
      hipError_t e = hipEventRecord (d->inputReady, st);
      if (e == hipSuccess) e = hipStreamWaitEvent (d->side, d->inputReady, 0);
      if (e != hipSuccess) { delete t; return mgHipFail (e, "mgQueryReadsDeviceAsync"); }
      if ((s = mgScanStart (d, slot, t->q, mgSurvivorGuess (ms->hasher, totalBases), &t->b, d->side))) { delete t; return s; }
      if ((e = hipEventRecord (d->scanned[slot], d->side)) != hipSuccess) { delete t; return mgHipFail (e, "mgQueryReadsDeviceAsync"); }
    }
  d->slotBusy[slot] = true; d->nextSlot = slot ^ 1; ++d->ticketsOut;
  *ticket = t;
  return MG_OK;
}

extern "C" MgStatus mgQueryReadsDeviceWait (void *ticket, U64 *nSeeds, void *stream)
{
  MgQueryTicket *t = (MgQueryTicket *) ticket;
  if (!t) { mgSetError ("mgQueryReadsDeviceWait: null ticket"); return MG_ERR_ARG; }
  MgDev *d = t->d;
  if (nSeeds) *nSeeds = 0;
  MgStatus s = MG_OK;
  U64 n = 0;
  /* the scan that Async started, and where its guess was too small the further ones, on the library's stream; then the lookups on the
     caller's (the scan is complete: the host has waited for it, so the caller's stream need not) */
  if (t->q.totalBases && t->q.nReads && !(s = mgScanRounds (d, t->slot, t->q, t->b.cap, &t->b, &n, d->side, d->scanned[t->slot])))
    { if (nSeeds) *nSeeds = n;
      s = mgSeedsOfScanned (0, d, t->b, n, t->dSeedIndex, t->dSeedPosF, t->dSeedRead, t->capacity, (hipStream_t) stream);
    }
  d->slotBusy[t->slot] = false; --d->ticketsOut;
  delete t;
  return s;
}
