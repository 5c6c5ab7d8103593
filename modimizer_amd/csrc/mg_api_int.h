/* mg_api_int.h — what the host glue behind the C ABI shares between its files: mg_runtime.hip (errors, device, profiler, hasher
 * parameters), mg_hostbatch.hip (host bytes in, host arrays out; the iterator facade), mg_modsetdev.hip (a Modset's device state) and
 * mg_reads.hip (a device batch of reads against a set).  Not installed, nothing in it is exported. */
#ifndef MG_API_INT_H
#define MG_API_INT_H
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include "mg_common.h"
#include "mg_internal.h"

/* the load a table is brought to before lookups (a probe that misses walks to the next empty slot, and a workgroup of the partitioned
   lookups waits for its longest walk).  Rounds 1-5 asked for 60 and got 35-60: the slot count was rounded up to a power of two (config 3:
   0.35).  With the slot count free the figure is the load: 60 cost config 3's bucket lookups 0.99 -> 1.41 ms; 40 is what they had. */
#define MG_LOOKUP_LOAD_PCT 40

/* grow-only device scratch */
struct MgArena {
  char *base = 0; size_t bytes = 0; size_t used = 0;
  MgStatus reserve (size_t need)
  { if (need <= bytes) return MG_OK;
    if (base) MG_HIP (hipFree (base));
    base = 0; bytes = 0;
    size_t want = need + need / 8 + (1 << 20);
    MG_HIP (hipMalloc ((void **) &base, want));
    bytes = want;
    return MG_OK;
  }
  /* the same for room that would be good to have: false, and no error sentence, where the device has none (the arena is then empty) */
  bool tryReserve (size_t need)
  { if (need <= bytes) return true;
    if (base) (void) hipFree (base);
    base = 0; bytes = 0;
    const size_t want = need + need / 8 + (1 << 20);
    if (hipMalloc ((void **) &base, want) != hipSuccess) { (void) hipGetLastError (); base = 0; return false; }
    bytes = want;
    return true;
  }
  void reset () { used = 0; }
  void *take (size_t n) { size_t a = mgAl256 (used); used = a + n; return base + a; }
  void release () { if (base) (void) hipFree (base); base = 0; bytes = used = 0; }
};

/* per-Modset device state (mg_modsetdev.hip) */
struct MgDev {
  MgTable t;
  MgArena arena;           /* the scratch of the call in flight (slot 0 of the query pipeline) */
  MgArena arena2;          /* slot 1: the scan of the NEXT query batch runs into it while the lookups of this one read slot 0's segments (mgQueryReadsDeviceAsync) */
  hipStream_t side = 0;    /* the stream those scans run on */
  hipEvent_t scanned[2] = { 0, 0 }, inputReady = 0;
  int ticketsOut = 0, nextSlot = 0; bool slotBusy[2] = { false, false };
  /* a bucketed add's value writer on a stream of the set's own, behind the add's merge kernel (mgTableAdd, MgValueAside): it reads the batch's k-mers
     and the add's rank records where the add left them, in one of the two arenas, so it has an event per arena.  valuePending[slot]: a writer was
     started on that arena and nobody has waited for it on the host yet; valueLast: the arena of the last one.  Only mgValueSettle looks at the events. */
  hipStream_t valueStream = 0; hipEvent_t valueDone[2] = { 0, 0 }, merged = 0; bool valuePending[2] = { false, false }; int valueLast = 0;
  U64 *hPin;               /* pinned host words the per-call counters come back into: a device-to-host copy into pageable memory
                              goes through the runtime's staging path, whose wake-up was seen to take 10 - 25 ms now and then */
  U32 hostIndexMax;        /* entries 1..hostIndexMax are present in the host index[] table */
  bool built;
  int device = -1;         /* the GPU the table lives on: the one that was current when it was built */
};

/* the verdict of a scan's counters (MG_COUNT_WORDS words) for the capacity it ran with: 0 and *n = its modimizers, or the capacity to scan again with */
static inline U64 mgScanRetryCap (const volatile U64 *c, U64 cap, U64 *n)
{ *n = c[0]; return (c[1] || c[0] > cap) ? c[3] : 0; }

MG_HIDDEN MgStatus mgCheckHasher (const Seqhash *sh);                      /* mg_runtime.hip */
MG_HIDDEN U64      mgSurvivorGuess (const Seqhash *sh, U64 totalBases);     /* mg_hostbatch.hip: the capacity a batch is first scanned with */
MG_HIDDEN void     mgUploadRelease (void);                                  /* mg_hostbatch.hip: mgUploadPack's staging, on every device */
MG_HIDDEN MgDev   *mgDevLookup (const Modset *ms);                          /* mg_modsetdev.hip, as the rest */
MG_HIDDEN MgStatus mgDevGet (Modset *ms, MgDev **out, hipStream_t st);      /* get (and bring up to date) the device state of ms */
MG_HIDDEN MgStatus mgDevRefuseInFlight (const MgDev *d);                    /* MG_ERR_ARG and its sentence while a query batch of the set is in flight */
static inline MgArena &mgArenaOf (MgDev *d, int slot) { return slot ? d->arena2 : d->arena; }
/* The one owner of a pending value writer.  Whoever reads or writes t.value makes its stream wait (MG_SETTLE_STREAM); whoever frees, resets or
   reallocates what the writer reads -- an arena, the table's arrays -- or rolls the add back waits on the host (MG_SETTLE_HOST).  slot: that
   arena's writer alone, -1: both. */
enum { MG_SETTLE_STREAM = 0, MG_SETTLE_HOST = 1 };
MG_HIDDEN MgStatus mgValueSettle (MgDev *d, hipStream_t st, int how, int slot = -1);
MG_HIDDEN MgStatus mgArenaOpen (MgDev *d, int slot, size_t need);           /* the arena for a new call: its writer waited for, reserved, reset */
MG_HIDDEN void     mgArenaTwin (MgDev *d, int slot);                        /* the other arena made as large as what this one's call took, if it is free and smaller */
MG_HIDDEN U64      mgAddChunkSize (void);
#define MG_ADD_CHUNK (mgAddChunkSize ())
/* liveSlot >= 0: dKmer (or segSrc) lives in that arena, which the caller sized for the insert's temporaries too; -1: the caller's own array, and the
   temporaries are taken from a reset arena 0.  asideByDefault: with MODGPU_VALUE_ASYNC unset the value writer goes off the caller's stream */
MG_HIDDEN MgStatus mgAddBatch (Modset *ms, MgDev *d, const U64 *dKmer, U64 n, U32 *dIndexOut, int withDepth,
                               int liveSlot, hipStream_t st, const MgHistReq *counted = 0, const MgSegSrc *segSrc = 0, bool asideByDefault = false);
extern "C" void mgHostBatchRelease (void);                                  /* mg_hostbatch.hip (exported) */
#endif
