/* mg_modsetdev.hip — a Modset's device state (MgDev): the registry of the sets that have a device table, its build from the host
 * arrays and the mirror of what the host appends, clear, merge, prune, the batch add and find, the way back to the host arrays
 * (modsetSyncToHost) and the device views.  The reference-compatible scalar API (layer 1) lives in mg_host.c and calls the mgHook*
 * functions defined here to keep the host arrays and the device table coherent.
 */
#include <unordered_map>
#include "mg_api_int.h"
#include "mg_xfer.h"

/* the calling thread on a modset's own GPU for the length of a scope (the scalar API's hooks and the mirror may be reached from a thread
   that has since moved to another GPU with mgSetDevice) */
struct MgOnDevice
{ int before = -1; bool moved = false;
  explicit MgOnDevice (int dev) { if (dev >= 0 && hipGetDevice (&before) == hipSuccess && before != dev) moved = hipSetDevice (dev) == hipSuccess; }
  ~MgOnDevice () { if (moved) (void) hipSetDevice (before); }
};

static std::mutex gRegLock;
static std::unordered_map<const Modset *, MgDev *> gReg;
extern "C" { volatile int mgLiveDeviceModsets = 0; }

MgDev *mgDevLookup (const Modset *ms)
{ std::lock_guard<std::mutex> g (gRegLock); auto it = gReg.find (ms); return it == gReg.end () ? 0 : it->second; }

/* ---- the pending value writer (MgDev.valueStream): its one owner ---- */
MgStatus mgValueSettle (MgDev *d, hipStream_t st, int how, int slot)
{
  for (int i = 0 ; i < 2 ; ++i)
    { if (!d->valuePending[i] || (slot >= 0 && i != slot)) continue;
      if (how == MG_SETTLE_HOST) { MG_HIP (hipEventSynchronize (d->valueDone[i])); d->valuePending[i] = false; }
      else MG_HIP (hipStreamWaitEvent (st, d->valueDone[i], 0));
    }
  return MG_OK;
}
MgStatus mgArenaOpen (MgDev *d, int slot, size_t need)
{
  MgStatus s = mgValueSettle (d, 0, MG_SETTLE_HOST, slot); if (s) return s;
  MgArena &ar = mgArenaOf (d, slot);
  if ((s = ar.reserve (need))) return s;
  ar.reset ();
  return MG_OK;
}
/* An add whose writer was left running in arena `slot` expects the set's next add in the other arena: that one is allocated now, in the call
   that allocated the first (the first add of a set, where every other allocation of the set is made too), not in the next call -- which then
   allocates and frees nothing, as it never did: a set's second add is as fast as its tenth.  The price is the second arena for a set that
   turns out to take one add only.  Failing to get it is not this call's failure, and leaves no error sentence: the next add
   asks once more and otherwise makes do with one arena (mgAddReadsDevice). */
void mgArenaTwin (MgDev *d, int slot)
{
  MgArena &ar = mgArenaOf (d, slot), &other = mgArenaOf (d, slot ^ 1);
  if (other.bytes >= ar.used || d->valuePending[slot ^ 1] || d->slotBusy[slot ^ 1]) return;
  (void) other.tryReserve (ar.used);
}
/* the writer's stream and events, made on first use */
static MgStatus mgValueStream (MgDev *d)
{
  if (d->valueStream) return MG_OK;
  /* Highest priority: the runtime hands out its few hardware queues per priority, and a stream of the default priority may be given the caller's
     own queue -- the writer then runs behind the caller's next kernels, not beside them.  (Not the lowest: DESIGN_EXPERIMENTS.md section R item 5.)
     Between the writer and the caller's own kernels the priority decides nothing: the writer's few workgroups are resident before the caller's
     next kernel arrives */
  int lo = 0, hi = 0; (void) hipDeviceGetStreamPriorityRange (&lo, &hi);
  MG_HIP (hipStreamCreateWithPriority (&d->valueStream, hipStreamNonBlocking, hi));
  for (int i = 0 ; i < 2 ; ++i) MG_HIP (hipEventCreateWithFlags (&d->valueDone[i], hipEventDisableTiming));
  MG_HIP (hipEventCreateWithFlags (&d->merged, hipEventDisableTiming));
  return MG_OK;
}

static void mgDevFree (MgDev *d)
{
  if (!d) return;
  MgOnDevice here (d->device);
  (void) mgValueSettle (d, 0, MG_SETTLE_HOST);         /* (a writer still reads an arena and writes value[]) */
  if (d->valueStream) { (void) hipStreamSynchronize (d->valueStream); (void) hipStreamDestroy (d->valueStream); }
  for (int i = 0 ; i < 2 ; ++i) if (d->valueDone[i]) (void) hipEventDestroy (d->valueDone[i]);
  if (d->merged) (void) hipEventDestroy (d->merged);
  if (d->hPin) (void) hipHostFree (d->hPin);
  if (d->built)
    { (void) hipFree (d->t.slots); (void) hipFree (d->t.value); (void) hipFree (d->t.occ); (void) hipFree (d->t.find8);
      (void) hipFree (d->t.baseDepth); (void) hipFree (d->t.counters); (void) hipFree (d->t.liveHist);
    }
  if (d->side) { (void) hipStreamSynchronize (d->side); (void) hipStreamDestroy (d->side); }      /* (a scan started by mgQueryReadsDeviceAsync and never waited for still writes into an arena) */
  d->arena.release (); d->arena2.release ();
  for (int i = 0 ; i < 2 ; ++i) if (d->scanned[i]) (void) hipEventDestroy (d->scanned[i]);
  if (d->inputReady) (void) hipEventDestroy (d->inputReady);
  delete d;
}

/* ms leaves the registry and its device state goes */
static void mgDevDrop (Modset *ms, MgDev *d)
{
  { std::lock_guard<std::mutex> g (gRegLock); gReg.erase (ms); mgLiveDeviceModsets = (int) gReg.size (); }
  mgDevFree (d);
}

/* MG_OK when the calling thread is on the GPU d's table lives on; else MG_ERR_ARG, with its sentence unless quiet */
static MgStatus mgDevOnCallersGpu (const MgDev *d, bool quiet = false)
{
  int cur = -1;
  if (hipGetDevice (&cur) == hipSuccess && cur == d->device) return MG_OK;
  if (!quiet) mgSetError ("this Modset's table lives on GPU %d, the calling thread is on GPU %d (mgSetDevice)", d->device, cur);
  return MG_ERR_ARG;
}

MgStatus mgDevRefuseInFlight (const MgDev *d)
{
  if (!d->ticketsOut) return MG_OK;
  mgSetError ("a query batch of this modset is in flight (mgQueryReadsDeviceAsync without its mgQueryReadsDeviceWait)");
  return MG_ERR_ARG;
}

static MgStatus mgDevBuild (Modset *ms, MgDev *d, hipStream_t st)
{
  MgTable &t = d->t;
  { MgStatus s0 = mgValueSettle (d, st, MG_SETTLE_HOST); if (s0) return s0; }      /* (a new MgDev has none pending) */
  if (ms->tableBits < 20 || ms->tableBits > 32)
    { mgSetError ("device modset supports table bits 20..32 (got %d)", ms->tableBits); return MG_ERR_ARG; }
  memset (&t, 0, sizeof (t));
  t.maxLog2Slots = ms->tableBits - 1;                 /* load <= 0.5 at the largest legal fill */
  t.kbits = 2 * ms->hasher->k;
  t.wantR = 4096;                                      /* 64 KiB of LDS per bucket, 1024-thread workgroups (measured best) */
  { const long r = mgKnobs ()->bucketR; if (r != MG_KNOB_UNSET && r >= 256) t.wantR = (U32) r; }     /* test knob */
  t.size = ms->size;
  t.pin = d->hPin + 24;                                /* (hPin: 32 words; 0-1 the add's counters, 8-23 the scans' counts) */
  U64 cap = (ms->tableSize >> 2);                      /* device arrays cover the largest legal size */
  MG_HIP (hipMalloc ((void **) &t.value, cap * sizeof (U64)));
  MG_HIP (hipMalloc ((void **) &t.baseDepth, cap * sizeof (U16)));
  MG_HIP (hipMalloc ((void **) &t.counters, 64));
  d->built = true;
  MG_HIP (hipMemsetAsync (t.baseDepth, 0, cap * sizeof (U16), st));
  MG_HIP (hipMemsetAsync (t.counters, 0, 64, st));
  { MgStatus s0 = mgTableEnsure (&t, ms->max, st); if (s0) return s0; }   /* slots sized to the content; grows on demand */
  t.max = 0; t.syncedMax = 0;
  t.baseZero = !ms->max;
  if (ms->max)
    { MG_HIP (hipStreamSynchronize (st));               /* (the memsets above: the team copies on streams of its own) */
      MgStatus s;
      if ((s = mgXferH2D (t.value, ms->value, ((size_t) ms->max + 1) * sizeof (U64)))) return s;
      if ((s = mgXferH2D (t.baseDepth, ms->depth, ((size_t) ms->max + 1) * sizeof (U16)))) return s;
      if ((s = mgTableLoadHost (&t, t.value, 1, ms->max, st))) return s;
      MG_HIP (hipStreamSynchronize (st));
      t.max = t.syncedMax = ms->max;
    }
  d->hostIndexMax = ms->max;
  return MG_OK;
}

MgStatus mgDevGet (Modset *ms, MgDev **out, hipStream_t st)
{
  MgStatus s = mgEnsureDevice (); if (s) return s;
  if (!ms || !ms->hasher) { mgSetError ("null Modset"); return MG_ERR_ARG; }
  if ((s = mgCheckHasher (ms->hasher))) return s;
  MgDev *d = mgDevLookup (ms);
  if (!d)
    { d = new MgDev (); d->built = false; d->hostIndexMax = 0; d->hPin = 0;
      if (hipGetDevice (&d->device) != hipSuccess) { delete d; return mgHipFail (hipGetLastError (), "hipGetDevice"); }
      if (hipHostMalloc ((void **) &d->hPin, 256, hipHostMallocDefault) != hipSuccess) { delete d; return mgHipFail (hipGetLastError (), "hipHostMalloc"); }
      if ((s = mgDevBuild (ms, d, st))) { mgDevFree (d); return s; }
      mgXferWarm ();                                       /* what is built on the device comes back through mg_xfer.hip: its streams are made meanwhile */
      std::lock_guard<std::mutex> g (gRegLock); gReg[ms] = d; mgLiveDeviceModsets = (int) gReg.size ();
    }
  else if ((s = mgDevOnCallersGpu (d))) return s;
  if (d->built && ms->max > d->t.max)
    { /* the host appended entries through the scalar API (modsetIndexFind isAdd): mirror them */
      U32 first = d->t.max + 1, last = ms->max;
      if (last >= (ms->tableSize >> 2)) { mgSetError ("modset max %u beyond table capacity", last); return MG_ERR_CAPACITY; }
      if ((s = mgValueSettle (d, st, MG_SETTLE_STREAM))) return s;      /* the copies below go behind the last add's values */
      MG_HIP (hipMemcpyAsync (d->t.value + first, ms->value + first, (size_t) (last - first + 1) * sizeof (U64), hipMemcpyHostToDevice, st));
      MG_HIP (hipMemcpyAsync (d->t.baseDepth + first, ms->depth + first, (size_t) (last - first + 1) * sizeof (U16), hipMemcpyHostToDevice, st));
      d->t.baseZero = false;
      /* room for them, as for a batch of as many -- unless a query batch is in flight, whose scan has counted its digits for the geometry
         the table has.  (The loader may still have to refit the geometry where a bucket overflows, mgTableLoadHost; the waiting batch's
         counts are then for another geometry, mgTableFindTakesPartition sees that and its lookups go by direct probes: correct, slower.) */
      if (!d->ticketsOut && (s = mgTableEnsure (&d->t, last - first + 1, st))) return s;
      if ((s = mgTableLoadHost (&d->t, d->t.value, first, last, st))) return s;
      MG_HIP (hipStreamSynchronize (st));
      d->t.max = d->t.syncedMax = last;
      if (d->hostIndexMax == first - 1) d->hostIndexMax = last;
    }
  d->t.size = ms->size;
  *out = d;
  return MG_OK;
}

extern "C" MgStatus mgModsetDeviceRelease (Modset *ms)
{
  MgDev *d = mgDevLookup (ms);
  if (!d) return MG_OK;
  MgStatus s = modsetSyncToHost (ms, 1);
  mgDevDrop (ms, d);
  return s;
}

extern "C" void mgModsetHostChanged (Modset *ms)
{
  MgDev *d = mgDevLookup (ms);
  if (d) mgDevDrop (ms, d);
}

extern "C" MgStatus mgModsetClear (Modset *ms, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  MgDev *d = mgDevLookup (ms);
  if (d) { MgStatus s = mgDevOnCallersGpu (d); if (s) return s; }
  /* Host arrays only hold what the host was given: with a device table, entries beyond
     syncedMax exist on the device alone and index[] is populated up to hostIndexMax. */
  U32 hostIndexed = d ? d->hostIndexMax : ms->max;
  U32 hostUsed = d ? d->t.syncedMax : ms->max;
  if (d)
    { MgTable &t = d->t;
      mgTableForget (&t, st);          /* buckets are re-initialised by whoever writes them next (no 8 GB memset) */
      if (!t.baseZero) MG_HIP (hipMemsetAsync (t.baseDepth, 0, ((size_t) (t.max > t.syncedMax ? t.max : t.syncedMax) + 1) * sizeof (U16), st));
      t.baseZero = true;
      t.max = t.syncedMax = 0;
      t.pendingDepth = false;
      d->hostIndexMax = 0;
    }
  if (hostIndexed) memset (ms->index, 0, ms->tableSize * sizeof (U32));
  if (hostUsed)
    { memset (ms->depth, 0, ((size_t) hostUsed + 1) * sizeof (U16));
      memset (ms->info, 0, (size_t) hostUsed + 1);
    }
  ms->max = 0;
  return MG_OK;
}

/* device forms of the whole-set passes, used when the modset lives on the device ------------- */

/* fold the pending device counts into baseDepth (afterwards baseDepth[i] IS depth[i]).  The callers that go on to REWRITE the host's depth[]
   wholesale from baseDepth (merge, prune) pass no `host`; one that leaves the host arrays alone (mgHookDeviceView, modsetSyncToHost) passes the
   Modset, and the pending counts reach its depth[]: depth[i] = min (65535, depth[i] + pending) -- the fold clears pendingDepth, so no later
   sync would (a sender of a rank-order merge was left with stale host depths) */
static MgStatus mgFoldCounts (MgDev *d, hipStream_t st, Modset *host = 0)
{
  MgTable &t = d->t;
  if (!t.max) return MG_OK;
  if (!t.pendingDepth) return MG_OK;                   /* nothing has counted since the last fold */
  MgStatus s = mgArenaOpen (d, 0, mgAl256 ((size_t) t.max * sizeof (U16)) + 4096); if (s) return s;      /* (no call is using the arena while a whole-set pass runs) */
  U16 *dDelta = (U16 *) d->arena.take ((size_t) t.max * sizeof (U16));
  s = mgTableExportDepth (&t, dDelta, st);
  MG_HIP (hipStreamSynchronize (st));
  if (!s && host) s = mgXferD2H (host->depth + 1, dDelta, (size_t) t.max * sizeof (U16), MG_XFER_SATADD16);      /* modutils.c:26, `pending` times */
  return s;
}

/* modset.c:106-128 with ms1 on the device.  The caller (mg_host.c) has checked the hashers and
 * regrown ms1's host arrays; ms2's host arrays are current.  Returns 0 on success. */
/* ms2's entries 1 .. n2 as device arrays (entry i at [i - 1]) merged into ms1, which is on the device */
static int mgMergeDeviceCore (Modset *ms1, MgDev *d, const U64 *dV2, const U16 *dD2, const U8 *dI2, U32 n2, hipStream_t st)
{
  MgTable &t = d->t;
  const U32 max1 = t.max;
  const char *const sorry = "device merge failed";
  if (mgValueSettle (d, st, MG_SETTLE_HOST)) return mgFailedWith (sorry);      /* value[] is read below by the transfer team's own streams */
  MgDevScratch scratch ("device merge");
  U8 *dI1; U32 *dIdx;
  const size_t cap1 = (size_t) max1 + n2 + 2;
  if (scratch.get (&dI1, cap1) || scratch.get (&dIdx, n2)) return -1;
  if (hipMemset (dI1, 0, cap1) || hipDeviceSynchronize ()) return mgFailedWith (sorry);
  if (mgXferH2D (dI1, ms1->info, (size_t) max1 + 1)) return mgFailedWith (sorry);
  /* ms2's values in ms2 index order: existing ones are found, new ones get max1+1, max1+2, ... (modset.c:120) */
  MgStatus as = mgAddBatch (ms1, d, dV2, n2, dIdx, 0, -1, st);
  if (as == MG_ERR_CAPACITY) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); exit (-1); }
  if (as) return mgFailedWith (sorry);
  t.baseZero = false; t.liveHistValid = false;
  if (mgTableMergeApply (dIdx, dD2, dI2, n2, t.baseDepth, dI1, st)) return mgFailedWith (sorry);
  if (hipStreamSynchronize (st)) return mgFailedWith (sorry);
  /* bring the host mirror up to date wholesale: values of the new entries, all depths and info */
  if (t.max > t.syncedMax)
    { if (mgXferD2H (ms1->value + t.syncedMax + 1, t.value + t.syncedMax + 1, (size_t) (t.max - t.syncedMax) * 8, MG_XFER_COPY)) return mgFailedWith (sorry);
      t.syncedMax = t.max;
    }
  if (mgXferD2H (ms1->depth, t.baseDepth, ((size_t) t.max + 1) * 2, MG_XFER_COPY)) return mgFailedWith (sorry);
  if (mgXferD2H (ms1->info, dI1, (size_t) t.max + 1, MG_XFER_COPY)) return mgFailedWith (sorry);
  ms1->depth[0] = 0;
  ms1->max = t.max;
  return 0;
}

extern "C" int mgHookMergeDevice (Modset *ms1, Modset *ms2)
{
  hipStream_t st = 0;
  MgDev *d; if (mgDevGet (ms1, &d, st)) return -1;
  const U32 n2 = ms2->max;
  if (mgFoldCounts (d, st)) return -1;
  if (!n2) return 0;
  MgDevScratch scratch ("device merge: the second set");
  U64 *dV2; U16 *dD2; U8 *dI2;
  if (scratch.get (&dV2, n2) || scratch.get (&dD2, n2) || scratch.get (&dI2, n2)) return -1;
  if (mgXferH2D (dV2, ms2->value + 1, (size_t) n2 * 8) || mgXferH2D (dD2, ms2->depth + 1, (size_t) n2 * 2) || mgXferH2D (dI2, ms2->info + 1, n2)) return mgFailedWith ("device merge failed");
  return mgMergeDeviceCore (ms1, d, dV2, dD2, dI2, n2, st);
}

/* the same with the second set's arrays already in device memory (what a rank receives from its peers over xGMI, mg_comm.hip):
   nothing of the second set crosses the host link */
extern "C" int mgHookMergeDeviceArrays (Modset *ms1, const U64 *dValue2, const U16 *dDepth2, const U8 *dInfo2, U32 n2)
{
  hipStream_t st = 0;
  MgDev *d; if (mgDevGet (ms1, &d, st)) return -1;
  if (mgFoldCounts (d, st)) return -1;
  if (!n2) return 0;
  return mgMergeDeviceCore (ms1, d, dValue2, dDepth2, dInfo2, n2, st);
}

/* modset.c:64-77 with ms on the device: survivors keep their order, the table is rebuilt from them */
extern "C" int mgHookPruneDevice (Modset *ms, int lo, int hi)
{
  hipStream_t st = 0;
  MgDev *d; if (mgDevGet (ms, &d, st)) return -1;
  MgTable &t = d->t;
  const U32 n = t.max;
  if (mgValueSettle (d, st, MG_SETTLE_HOST)) return -1;      /* value[] is compacted, then rewritten, on the default stream and by plain copies */
  if (mgFoldCounts (d, st)) return -1;
  /* values of device-only entries must reach the host before the arrays are rewritten?  No: the
     survivors are compacted on the device and copied back as a whole. */
  const char *const sorry = "device prune failed";
  MgDevScratch scratch ("device prune");
  U8 *dInfo, *dNewInfo; U64 *dNewValue; U16 *dNewDepth; char *dWork;
  if (scratch.get (&dInfo, (size_t) n + 1) || scratch.get (&dNewInfo, (size_t) n + 2) || scratch.get (&dNewValue, (size_t) n + 2)
      || scratch.get (&dNewDepth, (size_t) n + 2) || scratch.get (&dWork, mgTablePruneScratchBytes (n ? n : 1))) return -1;
  if (mgXferH2D (dInfo, ms->info, (size_t) n + 1)) return mgFailedWith (sorry);
  if (mgTablePrune (&t, dInfo, lo, hi, dNewValue, dNewDepth, dNewInfo, dWork, st)) return mgFailedWith (sorry);
  U64 c[2];
  if (hipMemcpyAsync (c, t.counters, 16, hipMemcpyDeviceToHost, st) || hipStreamSynchronize (st)) return mgFailedWith (sorry);
  const U32 m = (U32) c[0];
  /* new arrays replace the old ones on both sides */
  if (m)
    { t.baseZero = false; t.liveHistValid = false;
      if (hipMemcpy (t.value + 1, dNewValue + 1, (size_t) m * 8, hipMemcpyDeviceToDevice) || hipMemcpy (t.baseDepth + 1, dNewDepth + 1, (size_t) m * 2, hipMemcpyDeviceToDevice)
          || mgXferD2H (ms->value + 1, dNewValue + 1, (size_t) m * 8, MG_XFER_COPY) || mgXferD2H (ms->depth + 1, dNewDepth + 1, (size_t) m * 2, MG_XFER_COPY)
          || mgXferD2H (ms->info + 1, dNewInfo + 1, m, MG_XFER_COPY)) return mgFailedWith (sorry);
    }
  if (n > m && hipMemset (t.baseDepth + m + 1, 0, (size_t) (n - m) * 2)) return mgFailedWith (sorry);
  mgTableForget (&t, st);
  t.max = 0;
  if (mgTableEnsure (&t, m, st)) return mgFailedWith (sorry);
  if (m && mgTableLoadHost (&t, t.value, 1, m, st)) return mgFailedWith (sorry);
  if (hipStreamSynchronize (st)) return mgFailedWith (sorry);
  t.max = t.syncedMax = m;
  ms->max = m;
  d->hostIndexMax = 0;                 /* index[] is rebuilt (replayed) when somebody needs it */
  return 0;
}

/* hooks for mg_host.c */
extern "C" void mgHookDestroy (Modset *ms) { mgModsetHostChanged (ms); }
extern "C" void mgHookHostRewrote (Modset *ms) { mgModsetHostChanged (ms); }
extern "C" void mgHookNeedHostAll (Modset *ms, int wantIndex)
{
  MgDev *d = mgDevLookup (ms);
  if (!d) return;
  if (modsetSyncToHost (ms, wantIndex) != MG_OK)
    { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); exit (-1); }
}
extern "C" void mgHookNeedHost (Modset *ms, int wantIndex)
{
  MgDev *d = mgDevLookup (ms);
  if (!d) return;
  /* current when no entry, no index slot and no depth count is pending on the device (a batch that only re-hits
     existing k-mers leaves max alone but not depth[], which callers read and bump directly: modutils.c:26) */
  if (!d->t.pendingDepth && d->t.syncedMax == d->t.max && (!wantIndex || d->hostIndexMax >= d->t.max)) return;
  mgHookNeedHostAll (ms, wantIndex);
}
extern "C" int mgHookHasDevice (Modset *ms) { return mgDevLookup (ms) != 0; }

/* ---------------------------------------------------------------------------------------- */
/* batch insert / find                                                                        */

/* modimizers per insert pass (tokens are 31-bit ordinals); MODGPU_ADD_CHUNK shrinks it for tests */
U64 mgAddChunkSize (void)
{
  const long c = mgKnobs ()->addChunk;
  U64 v = c != MG_KNOB_UNSET && c > 0 ? (U64) c : ((U64) 1 << 30);
  if (v > ((U64) 1 << 30)) v = (U64) 1 << 30;
  return v;
}

/* asideSlot >= 0: the value writer may go onto the set's own stream; the batch and the scratch are in that arena and stay there */
static MgStatus mgAddChunk (Modset *ms, MgDev *d, const U64 *dKmer, U64 n, U32 *dIndexOut, int withDepth,
                            void *scratch, hipStream_t st, const MgHistReq *counted = 0, const MgSegSrc *segSrc = 0, int asideSlot = -1)
{
  MgTable &t = d->t;
  MgStatus s;
  MG_HIP (hipMemsetAsync (t.counters, 0, 16, st));
  MgValueAside aside = {};
  if (asideSlot >= 0)
    { if ((s = mgValueStream (d))) return s;
      if ((s = mgValueSettle (d, 0, MG_SETTLE_HOST, asideSlot))) return s;      /* (its event is recorded anew) */
      aside.stream = d->valueStream; aside.merged = d->merged; aside.done = d->valueDone[asideSlot];
    }
  else if ((s = mgValueSettle (d, st, MG_SETTLE_STREAM))) return s;              /* this add writes value[] on the caller's stream (either leg): behind the last add's writer */
  s = mgTableAdd (&t, dKmer, n, withDepth, scratch, st, counted, segSrc, asideSlot >= 0 ? &aside : 0);
  if (aside.launched) { d->valuePending[asideSlot] = true; d->valueLast = asideSlot; }
  if (s) return s;
  volatile U64 *c = d->hPin;
  MG_HIP (hipMemcpyAsync (d->hPin, t.counters, 16, hipMemcpyDeviceToHost, st));
  MG_HIP (hipStreamSynchronize (st));
  U64 newMax = (U64) t.max + c[0];
  if (c[1] || newMax >= t.size)
    { /* modset.c:58 */
      /* what the add had written by then goes out of the table again: the set answers as before the call, whichever lookup path is asked.
         (The refused add's values are beyond max and nobody's; its writer is waited for because the caller is about to hear that the call is over) */
      if ((s = mgValueSettle (d, st, MG_SETTLE_HOST))) return s;
      if ((s = mgTableRollback (&t, st))) return s;
      mgSetError ("hashTableSize %u is too small for %llu", t.size, (unsigned long long) newMax);
      return MG_ERR_CAPACITY;
    }
  t.max = (U32) newMax;
  ms->max = t.max;
  if (n >= 4096) t.newPct = (int) (c[0] * 100 / n);
  if (dIndexOut && (s = mgTableFind (&t, dKmer, n, dIndexOut, st))) return s;
  return MG_OK;
}

/* liveSlot >= 0: dKmer (or the segments) lives in that arena (mgAddReadsDevice), so the arena must not be reset or reallocated; the caller
 * reserved room for the temporaries taken here.  The value writer leaves the caller's stream where the knob says so (mg_knobs.h), for a batch
 * of one chunk; where the k-mers are the caller's own it is waited for before the call returns. */
MgStatus mgAddBatch (Modset *ms, MgDev *d, const U64 *dKmer, U64 n, U32 *dIndexOut, int withDepth,
                     int liveSlot, hipStream_t st, const MgHistReq *counted, const MgSegSrc *segSrc, bool asideByDefault)
{
  if (!n) return MG_OK;
  MgStatus s = mgDevRefuseInFlight (d); if (s) return s;
  U64 chunk = n < MG_ADD_CHUNK ? n : MG_ADD_CHUNK;
  if ((s = mgTableEnsure (&d->t, chunk, st))) return s;
  size_t need = mgTableAddScratchBytes (&d->t, chunk) + 4096;
  const int slot = liveSlot >= 0 ? liveSlot : 0;
  MgArena &ar = mgArenaOf (d, slot);
  if (liveSlot < 0) { if ((s = mgArenaOpen (d, 0, need))) return s; }
  else if (ar.bytes - ar.used < need)
    { mgSetError ("internal: arena too small for insert temporaries"); return MG_ERR_NOMEM; }
  void *scratch = ar.take (mgTableAddScratchBytes (&d->t, chunk));
  const long va = mgKnobs ()->valueAsync;
  /* (only the bucketed leg has a writer to move.  The direct leg writes value[] on the caller's stream, and mgAddChunk makes that stream wait for
     whatever an earlier add left running: after a clear that writer stores to the very entries this add assigns) */
  const bool aside = n <= chunk && mgTableUseBuckets (&d->t, chunk) && (va == MG_KNOB_UNSET ? asideByDefault : va == 1);
  for (U64 off = 0 ; off < n && !s ; off += chunk)
    { U64 m = n - off < chunk ? n - off : chunk;
      if (off) s = mgTableEnsure (&d->t, m, st);
      if (!s) s = mgAddChunk (ms, d, dKmer + off, m, dIndexOut ? dIndexOut + off : 0, withDepth, scratch, st,
                              (counted && n <= chunk) ? counted : 0,       /* the counts cover the whole batch */
                              n <= chunk ? segSrc : 0, aside ? slot : -1);
    }
  if (aside && liveSlot < 0) { MgStatus w = mgValueSettle (d, st, MG_SETTLE_HOST, slot); if (!s) s = w; }      /* dKmer is the caller's again when this returns */
  return s;
}

extern "C" MgStatus modsetAddBatchDevice (Modset *ms, const U64 *dKmer, U64 n, U32 *dIndexOut, int withDepth, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  MgDev *d; MgStatus s = mgDevGet (ms, &d, st); if (s) return s;
  return mgAddBatch (ms, d, dKmer, n, dIndexOut, withDepth, -1, st);
}

extern "C" MgStatus modsetFindBatchDevice (Modset *ms, const U64 *dKmer, U64 n, U32 *dIndexOut, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  MgDev *d; MgStatus s = mgDevGet (ms, &d, st); if (s) return s;
  d->t.loadPct = MG_LOOKUP_LOAD_PCT;
  if (d->t.slots && (s = mgTableEnsure (&d->t, 0, st))) return s;
  return mgTableFind (&d->t, dKmer, n, dIndexOut, st);
}

/* What the device holds and the host arrays do not yet: value[] of the entries past syncedMax, the pending depth counts, the
 * index[] layout.  The callers read those arrays themselves (modset.h:17-28; modutils.c:26,69,186-198; modset.c:79-88), so this IS
 * the last step of the path for them.  Everything moves through mg_xfer.hip's team (page-locked pieces, several copy streams, the
 * final memcpy / saturating add spread over the host's threads); the device-side temporaries (the 16-bit counts, the replayed
 * index[]) come out of the modset's grow-only arena, which no call is using while this one runs: nothing is allocated per call.
 * The host's depth[] stays the authority (a caller may have bumped it directly, modutils.c:26): pending counts are ADDED to it,
 * saturating -- the thread that empties a page-locked piece does that instead of a memcpy, at the same memory traffic. */
extern "C" MgStatus modsetSyncToHost (Modset *ms, int wantIndex)
{
  MgDev *d = mgDevLookup (ms);
  if (!d) return MG_OK;
  MgOnDevice here (d->device);
  MgTable &t = d->t;
  hipStream_t st = 0;
  MgStatus s;
  MG_HIP (hipDeviceSynchronize ());
  if ((s = mgValueSettle (d, st, MG_SETTLE_HOST))) return s;
  if (d->ticketsOut && (t.pendingDepth || (wantIndex && d->hostIndexMax < t.max)))
    { mgSetError ("a query batch of this modset is in flight (its scratch is what a sync would use)"); return MG_ERR_ARG; }
  if (t.max > t.syncedMax)
    { const U32 first = t.syncedMax + 1;
      if ((s = mgXferD2H (ms->value + first, t.value + first, (size_t) (t.max - first + 1) * sizeof (U64), MG_XFER_COPY))) return s;
      t.syncedMax = t.max;
    }
  ms->max = t.max;
  if ((s = mgFoldCounts (d, st, ms))) return s;
  if (wantIndex && d->hostIndexMax < t.max)
    { if ((s = mgArenaOpen (d, 0, mgAl256 (ms->tableSize * sizeof (U32)) + 4096))) return s;
      U32 *dIndex = (U32 *) d->arena.take (ms->tableSize * sizeof (U32));
      if ((s = mgTableReplayIndex (&t, mgMakeParams (ms->hasher), ms->tableBits, dIndex, st))) return s;
      MG_HIP (hipStreamSynchronize (st));
      if ((s = mgXferD2H (ms->index, dIndex, ms->tableSize * sizeof (U32), MG_XFER_COPY))) return s;
      d->hostIndexMax = t.max;
    }
  return MG_OK;
}

/* depth[] of ms has been remade from what the device counted elsewhere (modasm's read ingest, mg_rsdev.hip): the device table's own copy
   follows -- dDepth16[0 .. max] on the device -- instead of the whole table being dropped and rebuilt from the host arrays on its next use.
   No count is pending in the table (the caller synced before it started).  0 if there is no device table (nothing to do). */
extern "C" MgStatus mgModsetAdoptDepthDevice (Modset *ms, const U16 *dDepth16)
{
  MgDev *d = mgDevLookup (ms);
  if (!d || !d->built) return MG_OK;
  MgTable &t = d->t;
  if (t.pendingDepth || t.max != ms->max) { mgModsetHostChanged (ms); return MG_OK; }      /* (not in step with the host: start again from its arrays) */
  MG_HIP (hipMemcpy (t.baseDepth, dDepth16, ((size_t) t.max + 1) * sizeof (U16), hipMemcpyDeviceToDevice));
  t.baseZero = false; t.liveHistValid = false;
  return MG_OK;
}

/* ms's entries 1 .. max where the device table keeps them (value, depth with every pending count folded in), for a sender that wants
   them on the device anyway (mg_comm.hip); -1: no device table */
extern "C" int mgHookDeviceView (Modset *ms, const U64 **dValue1, const U16 **dDepth1, U32 *max)
{
  MgDev *d = mgDevLookup (ms);
  if (!d || !d->built || d->ticketsOut) return -1;
  if (mgDevOnCallersGpu (d, true)) return -1;      /* (a sender stages from the host then) */
  if (hipDeviceSynchronize () != hipSuccess || mgValueSettle (d, 0, MG_SETTLE_HOST) || mgFoldCounts (d, 0, ms)) return -1;
  *dValue1 = d->t.value + 1; *dDepth1 = d->t.baseDepth + 1; *max = d->t.max;
  return 0;
}

/* the same for the reports (mg_report.hip), the device table made first if the set has none yet (a set straight from modsetRead) */
extern "C" int mgHookDeviceViewMake (Modset *ms, const U64 **dValue1, const U16 **dDepth1, U32 *max)
{
  MgDev *d; if (mgDevGet (ms, &d, 0)) return -1;
  return mgHookDeviceView (ms, dValue1, dDepth1, max);
}

extern "C" U64 mgModsetDeviceSlots (Modset *ms) { MgDev *d = mgDevLookup (ms); return d && d->built ? d->t.nSlots : 0; }

extern "C" MgStatus mgTableCheckLayout (Modset *ms, U64 *out6)
{
  MgDev *d; MgStatus s = mgDevGet (ms, &d, 0); if (s) return s;
  MgDevScratch scratch ("mgTableCheckLayout");
  U64 *dOut;
  if (scratch.get (&dOut, 4)) return MG_ERR_HIP;
  s = mgTableLayoutCheck (&d->t, dOut, 0);
  if (!s && (hipMemcpy (out6, dOut, 32, hipMemcpyDeviceToHost) || hipMemcpy (out6 + 4, d->t.counters + 4, 16, hipMemcpyDeviceToHost))) s = MG_ERR_HIP;
  return s;
}

extern "C" MgStatus mgTableDiag (Modset *ms, U64 *out9)
{
  memset (out9, 0, 9 * sizeof (U64));
  MgDev *d = mgDevLookup (ms);
  if (!d || !d->built) return MG_OK;
  out9[0] = (U64) d->t.log2NB; out9[1] = d->t.R;
  for (int i = 0 ; i < 7 ; ++i) out9[2 + i] = d->t.diag[i];
  return MG_OK;
}

extern "C" MgStatus modsetDepthHistogramDevice (Modset *ms, U64 *dHist, void *stream)
{
  hipStream_t st = (hipStream_t) stream;
  MgDev *d; MgStatus s = mgDevGet (ms, &d, st); if (s) return s;
  return mgTableHistogram (&d->t, dHist, st);
}

/* the set's device table for a whole-set pass that only reads it (mg_modutils.hip): brought up to date with what the host appended, the
   device idle, no query batch in flight.  *t = 0: the set has no device table (no HIP call is made then) */
MgStatus mgModsetTableForPass (Modset *ms, MgTable **t)
{
  *t = 0;
  if (!ms) { mgSetError ("null Modset"); return MG_ERR_ARG; }
  if (!mgDevLookup (ms)) return MG_OK;
  MgDev *d; MgStatus s = mgDevGet (ms, &d, 0); if (s) return s;
  if (!d->built) return MG_OK;
  if ((s = mgDevRefuseInFlight (d))) return s;
  MG_HIP (hipDeviceSynchronize ());
  if ((s = mgValueSettle (d, 0, MG_SETTLE_HOST))) return s;
  ms->max = d->t.max;
  *t = &d->t;
  return MG_OK;
}
