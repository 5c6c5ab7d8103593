/* mg_tableadd.hip — mgTableAdd: a batch of k-mers into the device modset table (mg_table.hip: the layout and the two build paths).
 *
 * Here: the direct path's own kernels, the choice between the paths, what the bucketed leg decides before it launches anything (mgAddPlan,
 * mgAddTighten), the add's scratch (MgAddScratch, mgAddCarve: written once, for the size the caller is told and for the pointers), and
 * mgTableAdd itself, which launches in the order of the steps: the partition passes (mg_part.hip), the dedup kernel (mg_bucket.hip), the
 * ordered flag count (mg_rank.hip), the rank lookups and the merge kernel (mg_bucket.hip). */
#include "mg_table.h"

/* ======================================================================================== */
/* direct path                                                                                */

__global__ void mgTableInsertKernel (MgSlot *__restrict__ slots, MgGeom g, const U64 *__restrict__ kmer, U64 n,
                                     U32 *__restrict__ slotId, int withDepth, U64 *counters)
{
  U64 o = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; o < n ; o += stride)
    { const U64 m = mgMixK (kmer[o], g.kbits), key = m + 1;
      const U64 base = (U64) mgBucketOfM (m, g) * g.R;
      U32 at = mgHomeOfM (m, g);
      bool ok = false;
      for (U32 probes = 0 ; probes < g.R ; ++probes)
        { U64 cur = slots[base + at].key;          /* plain load: a stale "empty" is repaired by the CAS */
          if (cur == 0)
            { cur = atomicCAS ((unsigned long long *) &slots[base + at].key, 0ull, (unsigned long long) key);
              if (cur == 0) cur = key;
            }
          if (cur == key) { ok = true; break; }
          at = mgNextSlot (at, g.R);
        }
      if (!ok) { counters[1] = 1; slotId[o] = 0xffffffffu; continue; }
      const U64 s = base + at;
      U32 v = slots[s].ord;                        /* tokens only grow: a stale read is only ever too small */
      U32 tok = mgToken (o);
      if (v < tok) atomicMax (&slots[s].ord, tok); /* an assigned index (bit 31) is never below a token */
      if (withDepth)
        { /* the lanes of the wave that sit in the same slot as its first one add their number once: a run of one k-mer (64 consecutive
             modimizers of a poly-A stretch are one) would otherwise queue 64 atomics on one word -- 12 ns per occurrence */
          const U64 s0 = ((U64) (U32) __builtin_amdgcn_readfirstlane ((int) (U32) (s >> 32)) << 32) | (U32) __builtin_amdgcn_readfirstlane ((int) (U32) s);
          const bool mine = s == s0;
          const U64 grp = __ballot (mine);
          if (!mine) atomicAdd (&slots[s].cnt, 1u);
          else if ((threadIdx.x & 63) == (U32) __builtin_ctzll (grp)) atomicAdd (&slots[s].cnt, (U32) __popcll (grp));
        }
      slotId[o] = (U32) s;
    }
}

/* flags[o] = 1: the slot's token is this occurrence's, i.e. it is the first occurrence of a k-mer new to the table */
__global__ __launch_bounds__ (256)
void mgDirectFlagKernel (const MgSlot *__restrict__ slots, const U32 *__restrict__ slotId, U64 n,
                         unsigned char *__restrict__ flags)
{
  U64 o = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; o < n ; o += stride)
    { U32 s = slotId[o];
      flags[o] = (s != 0xffffffffu && slots[s].ord == mgToken (o)) ? 1 : 0;
    }
}

/* occ[] is kept exact only by the bucketed path and the loader; the direct path marks buckets non-empty */
__global__ void mgMarkOccKernel (MgGeom g, const U64 *__restrict__ kmer, U64 n, U32 *__restrict__ occ)
{
  U64 o = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; o < n ; o += stride)
    { U32 b = mgBucketOfM (mgMixK (kmer[o], g.kbits), g);
      if (!occ[b]) occ[b] = 1;
    }
}

MgStatus mgTableMarkOccupied (MgTable *t, const U64 *dKmer, U64 n, hipStream_t st)
{
  MG_LAUNCH (MG_K_TABLE_FLAG, st, mgMarkOccKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, mgGeomOf (t), dKmer, n, t->occ);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

/* ======================================================================================== */
/* the choice between the paths, and the bucketed path's plan                                 */

/* the split of oversize buckets: occurrences above which a bucket is split, occurrences of a chunk at least */
static void mgHotKnobs (U32 *split, U32 *chunk)
{
  const MgKnobs *k = mgKnobs ();                             /* test knob "split,chunk": small values send ordinary buckets through the split path */
  U32 a = MG_HOT_SPLIT_DEFAULT, b = MG_HOT_CHUNK_DEFAULT;
  if (k->hotSplit != MG_KNOB_UNSET && k->hotSplit > 0)
    { a = (U32) k->hotSplit; b = k->hotChunk != MG_KNOB_UNSET && k->hotChunk > 0 ? (U32) k->hotChunk : a / 4; }
  if (b < 64) b = 64;
  if (a < b) a = b;
  *split = a; *chunk = b;
}
static U64 mgHotItemsCap (U64 n) { U32 sp, ch; mgHotKnobs (&sp, &ch); return n / ch + n / sp + 16; }


static int mgPathOverride (void)
{
  const long c = mgKnobs ()->tablePath;                       /* test knob: the first letter of "direct" / "bucket" */
  return c == 'd' ? 1 : (c == 'b' ? 2 : 0);
}

bool mgTableUseBuckets (const MgTable *t, U64 n)
{
  int ov = mgPathOverride ();
  if (ov == 1) return false;
  if (ov == 2) return true;
  /* a batch of a million or so: the bucketed path's dozen launches and its per-bucket lists cost 0.43 ms whatever the size, the atomics
     0.1 ms + 0.19 ms per million (tools/size_sweep_probe.py: 0.78 M modimizers 0.30 against 0.43 ms, 3.1 M 0.68 against 0.45) */
  if (n < 1500000) return false;
  return n >= t->nSlots / 16;           /* streaming every touched bucket twice beats ~100 ps/modimizer of atomics */
}

/* did the scan count the digits of the first partition pass, for exactly this table geometry? */
static bool mgCountedFits (const MgTable *t, const MgHistReq *counted)
{ return counted && counted->binCount && counted->log2NB == t->log2NB && counted->kbits == t->kbits && !counted->hiB; }

/* can mgTableAdd read this batch from the scan's segments?  Only the bucketed path does, and its first pass then
   needs the digit counts the scan made */
bool mgTableAddTakesSegments (const MgTable *t, U64 n, const MgHistReq *counted)
{
  const int off = mgKnobs ()->noSegmentInput == 1;   /* test knob: always compact first */
  return !off && n && mgTableUseBuckets (t, n) && mgCountedFits (t, counted);
}

#define MG_TIGHT_PCT_DEFAULT 70      /* see MgTable.tightPct.  80 is 0.06 ms a step faster still on config 2 (DESIGN_EXPERIMENTS.md section L); 70 is what the full-size
                                        parity cases (tests/fullsize_whole.py) force as their other geometry, and they expect the default to be no tighter */
#define MG_TIGHT_PCT_CLAIMS 50       /* the same with MODGPU_MERGE_PLACE=0: the merge kernel's claims pay for the load */
#define MG_TIGHT_MIN_R 1024u         /* a bucket keeps room for the spread of a later add's share around its mean (mgTableEnsure sizes by the mean) */

/* What mgTableAdd's bucketed leg decides before it launches anything.  Every rule, and every knob that feeds one, is in mgAddPlan and nowhere else:
   the launches read the plan. */
struct MgAddPlan {
  int hiB, loB;                    /* the bucket id's coarse (high) and fine (low) digit, each <= 9 bits */
  MgPartFmt f; bool packed;        /* the partition's element format: one packed 8-byte word? */
  bool digitBytes;                 /* the first pass leaves every element's fine digit in a byte beside it, for the second pass's counts */
  int markDup, slotShift, place;   /* what MgBucketArgs says of them */
  bool tighten; int tightPct;      /* after the dedup kernel, bring R down to what the entries need at this load (mgAddTighten) */
  int sliceShift; U32 nSlices;     /* the rank lookups' slices of the ordinal range */
  U32 hotSplit, hotChunk;          /* the split of oversize buckets (mgHotKnobs) */
};
static void mgAddPlan (const MgTable *t, U64 n, bool wasEmpty, MgAddPlan *p)
{
  const U64 NB = (U64) 1 << t->log2NB;
  mgPartSplit (t->log2NB, &p->hiB, &p->loB);
  /* element format: one packed 8-byte word when the mixed k-mer without its coarse digit and the ordinal fit in 64 bits */
  p->f = mgPartFmtOf (t, n, p->hiB);
  { const int packEnv = mgKnobs ()->partPacked == MG_KNOB_UNSET ? 1 : (int) mgKnobs ()->partPacked;   /* test knob: 0 forces the wide format */
    p->packed = packEnv && mgPartFmtFits (t, p->f);
  }
  /* digit bytes: the second pass counts 156 MB of bytes instead of reading 1.25 GB of elements twice */
  p->digitBytes = p->loB && p->loB <= 8 && mgKnobs ()->partDigits != 0;
  mgHotKnobs (&p->hotSplit, &p->hotChunk);
  /* flag polarity from what the previous bucketed add saw (MgTable.newPct: new entries per 100 modimizers) */
  { const int polEnv = mgKnobs ()->flagPolarity == MG_KNOB_UNSET ? -1 : (int) mgKnobs ()->flagPolarity;   /* test knob: 0 / 1 force it */
    p->markDup = polEnv >= 0 ? (polEnv ? 1 : 0) : (t->newPct > 50 ? 1 : 0);
  }
  /* the merge kernel takes the slots from the dedup kernel when the buckets will be more than half full (there its
     probing costs more than the dedup kernel's extra work: a 12.5 Gbp block at load 0.62 gains 0.4 ms, config 2 at 0.38
     nothing); the load is estimated from the share of new k-mers the previous add saw */
  const U64 expectNew = t->newPct > 0 ? n * (U64) t->newPct / 100 : n;
  { const int slotEnv = mgKnobs ()->mergeSlots == MG_KNOB_UNSET ? -1 : (int) mgKnobs ()->mergeSlots;   /* test knob: 0 / 1 force it */
    const bool dense = ((U64) t->max + expectNew) * 2 > t->nSlots;
    p->slotShift = (t->kbits <= MG_SLOT_SHIFT && (slotEnv >= 0 ? slotEnv != 0 : dense)) ? MG_SLOT_SHIFT : 0;
  }
  /* An add into an EMPTY table (a set built from one batch: every step of the benchmarks, the first file of a run) does not know its
     entries until the dedup kernel has counted them -- the table was sized from the batch's occurrences, an upper bound -- and nothing is
     in the table yet, so its geometry is still free: after the dedup kernel R can be brought down to what the entries need at the tight
     load, and the merge kernel streams back that much less.  The price: the dedup kernel's image is then not the merge kernel's, so no
     slots are carried over and the merge kernel claims its own -- and a workgroup waits for its LONGEST probe chain (8 links at load 0.38,
     30 at 0.6, 80 at 0.75; profiles/r06_ab_table_geometry.txt: the merge kernel 1.07 / 1.20 / 1.44 / 2.5 ms at tight loads 50 / 60 / 70 / 80
     per cent on config 2, against 0.65 ms with carried slots at load 0.77).  So the table is only tightened where that pays: when the share
     of new k-mers the previous add saw (newPct; unknown: all new) says the entries will leave a quarter of the slots and more unused even at
     the tight load -- reads of deep coverage with few errors (config 5: a sixth of the modimizers are new; 4.3 -> 1.07 GB of bucket images). */
  int tightPct = t->tightPct ? t->tightPct : MG_TIGHT_PCT_CLAIMS;      /* (MG_TIGHT_PCT_DEFAULT below, where the merge kernel places by scan) */
  { const long tk = mgKnobs ()->tightLoad; if (tk != MG_KNOB_UNSET && tk >= 0 && tk <= 95) tightPct = (int) tk; }
  bool tighten = wasEmpty && tightPct > 0 && t->log2NB > 0 && t->pin;
  if (tighten && mgKnobs ()->tightLoad == MG_KNOB_UNSET)          /* (the knob forces it: tests, sweeps) */
    tighten = expectNew * 100 / (U64) tightPct < t->nSlots - t->nSlots / 4;
  /* a bucket that is empty before the add is laid out by prefix scan in the merge kernel (mgPlaceStarts): no probe whatever the load,
     so an add into an empty table has no use for the dedup kernel's slots, and the tightening costs the merge kernel nothing: it is
     done whenever the table was empty and the scan is on (DESIGN_EXPERIMENTS.md section L).  Only lists without carried slots go
     through the scan (the kernel checks a.slotShift): a later add that carries slots puts an empty bucket's entries where they say. */
  { const long pk = mgKnobs ()->mergePlace;                        /* MODGPU_MERGE_PLACE: 0 = claims everywhere, 1 = the scan for every fresh bucket, unset = the rule below */
    p->place = pk == MG_KNOB_UNSET ? 1 : (pk != 0);
    /* Left to itself the placement is for lists the kernel's spill-free instance takes whole (the uniques fetched ahead: MG_MERGE_PREFETCH
       per thread).  Where the buckets' lists will be longer -- a config-4 block: 2500 uniques per bucket and 1024 threads -- the add goes
       as before (carried slots; 11.06 ms a step against 11.16-11.44 with the scan's larger instance and the table at load 0.8).
       The lists' length is estimated from the share of new k-mers the previous add saw; the FIRST add a table ever sees has none to go by,
       is taken as all new (n / NB = 0.75 R uniques per bucket: over the limit at every default geometry) and so goes as before too: the
       scan and the tightening start with the second set a process builds from empty, which is every timed step of the benchmarks but not
       the first file of a run.  Which instance fits is known exactly only after the dedup kernel -- too late for the choice between
       the scan and carried slots, which the dedup kernel's own instance depends on. */
    if (pk == MG_KNOB_UNSET && expectNew / NB * 115 / 100 > (U64) MG_MERGE_PREFETCH * mgBucketThreads (t->R, 0)) p->place = 0;   /* (0: this rule has never looked at MODGPU_BUCKET_T) */
    if (p->place && wasEmpty) p->slotShift = 0;
    if (p->place && mgKnobs ()->tightLoad == MG_KNOB_UNSET)
      { if (!t->tightPct) tightPct = MG_TIGHT_PCT_DEFAULT;
        tighten = wasEmpty && tightPct > 0 && t->log2NB > 0 && t->pin;
      }
  }
  if (tighten) p->slotShift = 0;
  /* slices of the ordinal range for the rank lookups: 2^sliceShift ordinals each (2^22: 1 MiB of rank records, and a
     bucket's share of a slice is usually shorter than a wave), at most MG_RANK_GROUPS - 1 of them */
  { p->sliceShift = 22;
    /* a batch much smaller than the headline's would be three or four slices -- and the lookup kernel gives a slice to an XCD, so half
       the chip would idle (1 Gbp batches, as the file entry points make them: the rank lookups 0.31 ms of 1.39, with 2^18-ordinal slices
       0.11 of 1.11): smaller slices until there are 32 of them */
    while (p->sliceShift > 16 && ((n - 1) >> p->sliceShift) + 1 < 32) --p->sliceShift;
    if (mgKnobs ()->rankSliceShift != MG_KNOB_UNSET) p->sliceShift = (int) mgKnobs ()->rankSliceShift;   /* dev knob */
    while (((n - 1) >> p->sliceShift) + 1 > (U64) (MG_RANK_GROUPS - 1)) ++p->sliceShift;
    p->nSlices = (U32) (((n - 1) >> p->sliceShift) + 1);
  }
  p->tighten = tighten; p->tightPct = tightPct;
}
/* The tightening of an add into an empty table (mgAddPlan), between the dedup kernel and the merge: the entries and the fullest bucket's are counted -- the stream
   is waited for -- and R comes down to what they need at load tightPct.  *fullest: the fullest bucket's entries, unless a bucket overflowed. */
static MgStatus mgAddTighten (MgTable *t, int tightPct, const U32 *uniqCount, U64 *fullest, hipStream_t st)
{
  const U64 NB = (U64) 1 << t->log2NB;
  { MgStatus s = mgUniqStats (uniqCount, (U32) NB, (unsigned long long *) (t->counters + 2), st); if (s) return s; }
  MG_HIP (hipMemcpyAsync (t->pin, t->counters + 1, 24, hipMemcpyDeviceToHost, st));      /* overflow flag, entries, the fullest bucket's */
  MG_HIP (hipStreamSynchronize (st));
  const U64 over = t->pin[0], U = t->pin[1], M = t->pin[2];
  if (over) return MG_OK;
  *fullest = M;
  U64 Rn = (U * 100 / ((U64) NB * (U64) tightPct) + 1 + MG_R_QUANTUM - 1) / MG_R_QUANTUM * MG_R_QUANTUM;
  const U64 Rfit = (M + M / 8 + 16 + MG_R_QUANTUM - 1) / MG_R_QUANTUM * MG_R_QUANTUM;      /* the fullest bucket at load 0.89 at most */
  if (Rn < Rfit) Rn = Rfit;
  if (Rn < MG_TIGHT_MIN_R) Rn = MG_TIGHT_MIN_R;
  if (Rn < t->R) mgTableSetGeom (t, t->log2NB, (U32) Rn);
  return MG_OK;
}

/* ======================================================================================== */
/* the add's scratch: the rank buffers (mgRankCarve), then the direct leg's slotId[n] or the bucketed leg's arrays */

struct MgAddScratch {
  U64 *kA; U32 *tA;                          /* [n] the first partition pass's output where there are two */
  U64 *kB; U32 *tB, *cB;                     /* [n] the elements by bucket; the dedup kernel's lists in place over them (MgBucketArgs.pK, pT, pC) */
  U64 *fineStart; unsigned long long *fineCursor; U64 *spare64; U32 *fineCount, *uniqCount;   /* per bucket (spare64: unused, its bytes stay in the layout) */
  U64 *coarseStart; unsigned long long *coarseCursor; U64 *whole; U32 *coarseCount;           /* per coarse bin; whole: the batch as one segment */
  U32 *chunkBase;                            /* the partition's chunks per segment, and behind them the segment of every chunk */
  unsigned short *sliceOff;                  /* MgBucketArgs.sliceOff */
  MgSubSeg *subSeg;                          /* the segment cursor at every sub-chunk */
  U64 *hotItems; U32 *hotBuckets; unsigned long long *hotCount;   /* the oversize buckets (MgBucketArgs) */
};
/* the bucketed leg's arrays for a batch of n into a table of NB buckets, from base on; returns their bytes.  base 0: only measures (s may be 0 too) */
static size_t mgAddCarve (void *base, U64 n, U64 NB, MgAddScratch *s)
{
  MgAddScratch a; size_t at = 0;
  const U64 bins = MG_PART_MAXBINS, hot = mgHotItemsCap (n);
  a.kA = mgCarve<U64> (base, &at, n);
  a.tA = mgCarve<U32> (base, &at, n);
  a.kB = mgCarve<U64> (base, &at, n);
  a.tB = mgCarve<U32> (base, &at, n);
  a.cB = mgCarve<U32> (base, &at, n);
  a.fineStart = mgCarve<U64> (base, &at, NB + 2);
  a.fineCursor = mgCarve<unsigned long long> (base, &at, NB + 2 + bins * 16);
  a.spare64 = mgCarve<U64> (base, &at, NB + 2);
  a.fineCount = mgCarve<U32> (base, &at, NB + 2);
  a.uniqCount = mgCarve<U32> (base, &at, NB + 2);
  a.coarseStart = mgCarve<U64> (base, &at, bins + 2);
  a.coarseCursor = mgCarve<unsigned long long> (base, &at, (bins + 2) * 16);
  a.whole = mgCarve<U64> (base, &at, bins + 2);
  a.coarseCount = mgCarve<U32> (base, &at, bins + 2);
  a.chunkBase = mgCarve<U32> (base, &at, bins + 2 + n / MG_PART_CHUNK + bins + 2);
  a.sliceOff = mgCarve<unsigned short> (base, &at, (U64) (MG_RANK_GROUPS + 2) * NB);
  a.subSeg = mgCarve<MgSubSeg> (base, &at, n / MG_PART_SUB + 2);
  a.hotItems = mgCarve<U64> (base, &at, hot);
  a.hotBuckets = mgCarve<U32> (base, &at, hot);
  a.hotCount = mgCarve<unsigned long long> (base, &at, 32);
  if (s) *s = a;
  return at;
}

/* scratch needed by mgTableAdd for a batch of n: the larger leg's, with the most buckets a table has (it may grow between passes of one call) */
size_t mgTableAddScratchBytes (const MgTable *t, U64 n)
{
  (void) t;
  const size_t direct = mgAl256 (n * sizeof (U32)), part = mgAddCarve (0, n, (U64) 1 << 18, 0);
  return mgRankCarve (0, n, 0) + (direct > part ? direct : part) + 4096;
}

/* insert a batch (ordinal order = array order); counters[0] = number of new entries afterwards */
MgStatus mgTableAdd (MgTable *t, const U64 *dKmer, U64 n, int withDepth, void *scratch, hipStream_t st,
                     const MgHistReq *counted, const MgSegSrc *segSrc, MgValueAside *aside)
{
  if (aside) aside->launched = false;
  if (!n) return MG_OK;
  if ((uintptr_t) scratch & 255) { mgSetError ("internal: the insert's scratch is not 256-byte aligned"); return MG_ERR_ARG; }      /* (mgRankRecordKernel reads flags[] 16 bytes at a time) */
  if (segSrc && !mgTableAddTakesSegments (t, n, counted)) { mgSetError ("internal: this insert needs the dense k-mers"); return MG_ERR_ARG; }
  t->liveHistValid = false;                          /* set again below if this add is the set's only one */
  if (withDepth) t->pendingDepth = true;
  const bool wasEmpty = t->empty && t->max == 0;
  t->empty = false; ++t->version;
  MgGeom g = mgGeomOf (t);
  const bool buckets = mgTableUseBuckets (t, n);
  const U64 NB = (U64) 1 << t->log2NB;
  MgRankBufs rank; MgAddScratch w;
  char *const legBase = (char *) scratch + mgRankCarve (scratch, n, &rank);
  const size_t end = (size_t) (legBase - (char *) scratch) + (buckets ? mgAddCarve (legBase, n, NB, &w) : mgAl256 (n * sizeof (U32)));
  if (end > mgTableAddScratchBytes (t, n))
    { mgSetError ("internal: the insert's scratch layout (%zu bytes) passes the size its caller was told (%zu)", end, mgTableAddScratchBytes (t, n)); return MG_ERR_ARG; }
  MgStatus s;

  if (!buckets)
    { U32 *slotId = (U32 *) legBase;
      if (aside) { mgSetError ("internal: the direct insert has no value writer to run aside"); return MG_ERR_ARG; }      /* (it writes value[] on st: the caller decides by mgTableUseBuckets too, and orders st itself) */
      if ((s = mgTableClean (t, st))) return s;
      MG_LAUNCH (MG_K_TABLE_INSERT, st, mgTableInsertKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, t->slots, g, dKmer, n, slotId, withDepth, t->counters);
      MG_LAUNCH (MG_K_TABLE_FLAG, st, mgDirectFlagKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, t->slots, slotId, n, rank.flags);
      if ((s = mgRankCount (t, rank, n, st)) || (s = mgRankAssignDirect (t, rank, dKmer, slotId, n, st))) return s;
      MG_HIP (hipGetLastError ());
      return mgTableMarkOccupied (t, dKmer, n, st);
    }

  /* ---- bucketed ---- */
  MgAddPlan plan;
  mgAddPlan (t, n, wasEmpty, &plan);
  const int hiB = plan.hiB, loB = plan.loB;
  const U32 *pre = mgCountedFits (t, counted) ? counted->binCount : 0;
  U64 segInit[2] = { 0, n };
  MG_HIP (hipMemcpyAsync (w.whole, segInit, 16, hipMemcpyHostToDevice, st));
  MgPartPassArgs p1 = {};                /* the first pass: the batch, dense or in the scan's segments, by the coarse digit -- the only digit of a table of few buckets */
  p1.inMode = segSrc ? MG_EL_SEG : MG_EL_DENSE; p1.packed = plan.packed; p1.f = plan.f; p1.kIn = dKmer; p1.n = n; p1.segStart = w.whole; p1.nSeg = 1;
  p1.nBins = (U32) 1 << hiB; p1.chunkBase = w.chunkBase; p1.counted = pre; p1.segSrc = segSrc; p1.subSeg = w.subSeg;
  if (!loB)
    { p1.kOut = w.kB; p1.tOut = w.tB; p1.binStart = w.fineStart; p1.cursor = w.fineCursor; p1.binCount = w.fineCount;
      if ((s = mgPartPass (t, p1, st))) return s;
    }
  else
    { /* the first pass leaves every element's fine digit in a byte beside it (in w.cB, which the dedup kernel only writes later) */
      unsigned char *digits = plan.digitBytes ? reinterpret_cast<unsigned char *> (w.cB) : 0;
      p1.shift = loB; p1.kOut = w.kA; p1.tOut = w.tA; p1.binStart = w.coarseStart; p1.cursor = w.coarseCursor; p1.binCount = w.coarseCount;
      p1.digitOut = digits; p1.nextBins = (U32) 1 << loB;
      if ((s = mgPartPass (t, p1, st))) return s;
      MgPartPassArgs p2 = {};            /* the second pass: every coarse bin by the fine digit, into the buckets */
      p2.inMode = plan.packed ? MG_EL_PACKED : MG_EL_WIDE; p2.packed = plan.packed; p2.f = plan.f; p2.kIn = w.kA; p2.tIn = w.tA; p2.n = n; p2.segStart = w.coarseStart; p2.nSeg = (U32) 1 << hiB;
      p2.nBins = (U32) 1 << loB; p2.kOut = w.kB; p2.tOut = w.tB; p2.binStart = w.fineStart; p2.cursor = w.fineCursor; p2.binCount = w.fineCount; p2.chunkBase = w.chunkBase;
      p2.digitIn = digits;
      if ((s = mgPartPass (t, p2, st))) return s;
    }

  MG_HIP (hipMemsetAsync (rank.flags, plan.markDup ? 1 : 0, n, st));
  MgBucketArgs a;
  a.slots = t->slots; a.g = g; a.nBuckets = (U32) NB; a.bucketStart = w.fineStart;
  a.pK = w.kB; a.pT = w.tB; a.pC = w.cB; a.uniqCount = w.uniqCount; a.occ = t->occ; a.flags = rank.flags;
  a.grp = rank.grp; a.baseMax = t->max; a.size = t->size; a.withDepth = withDepth;
  a.markDup = plan.markDup; a.slotShift = plan.slotShift; a.place = plan.place;
  a.sliceShift = plan.sliceShift; a.nSlices = plan.nSlices; a.sliceOff = w.sliceOff;
  a.hotSplit = plan.hotSplit; a.hotChunk = plan.hotChunk; a.hotItems = w.hotItems; a.hotCount = w.hotCount; a.hotBuckets = w.hotBuckets;
  a.counters = t->counters; a.f = plan.f;
#ifdef MG_ABLATE
  { const long dbg = mgKnobs ()->bucketDebug; a.debug = dbg != MG_KNOB_UNSET ? (int) dbg : 0; }
#endif
  /* depth histogram on the fly: possible when this add builds the whole set (empty before, no host depths) */
  const bool track = t->max == 0 && t->baseZero;
  a.liveHist = 0;
  if (track)
    { if (!t->liveHist) MG_HIP (hipMalloc ((void **) &t->liveHist, 65536 * sizeof (U64)));
      MG_HIP (hipMemsetAsync (t->liveHist, 0, 65536 * sizeof (U64), st));
      a.liveHist = (unsigned long long *) t->liveHist;
    }
  t->liveHistValid = track;
  size_t lds = mgMergeLdsBytes (t->R);
  { const size_t ldsDedup = (size_t) t->R * 16 + MG_RANK_GROUPS * 4; if (ldsDedup > lds) lds = ldsDedup; }
  const int bThreadsEnv = mgKnobs ()->bucketT == MG_KNOB_UNSET ? 0 : (int) mgKnobs ()->bucketT;
  const unsigned bThreads = mgBucketThreads (t->R, bThreadsEnv);
  U32 perBlock;
  const unsigned bGrid = mgBucketGrid (NB, &perBlock);

  if ((s = mgBucketDedup (a, plan.packed, bThreads, bGrid, perBlock, lds, st))) return s;
  U64 fullest = t->R;                                  /* the longest list a bucket may have: not known unless the tightening counts it */
  if (plan.tighten)
    { if ((s = mgAddTighten (t, plan.tightPct, w.uniqCount, &fullest, st))) return s;
      if (t->R != a.g.R) { a.g = mgGeomOf (t); lds = mgMergeLdsBytes (t->R); }
    }
  /* index assignment in two halves.  The rank records are all the rest of the add needs; value[] is read by nobody before the caller looks at the
     set, so with `aside` its writer -- a plain stream over 2 GB -- goes behind the merge kernel onto a stream of its own, where it runs beside
     whatever the caller starts next: the scan of the next batch, which leaves the memory path idle.  (Beside the lookups or the merge of this add
     it cost more than it hid: they want the memory path themselves.) */
  if ((s = mgRankCount (t, rank, n, st)) || (s = mgRankRecord (rank, n, st))) return s;
  if (!aside && (s = mgWriteValues (t, rank.grp, dKmer, segSrc, w.subSeg, n, false, st))) return s;
  if ((s = mgRankLookup (a, st))) return s;
  if ((s = mgBucketMerge (a, fullest, bThreads, bGrid, perBlock, lds, st))) return s;
  MG_HIP (hipGetLastError ());
  if (aside)
    { MG_HIP (hipEventRecord (aside->merged, st));
      MG_HIP (hipStreamWaitEvent (aside->stream, aside->merged, 0));
      if ((s = mgWriteValues (t, rank.grp, dKmer, segSrc, w.subSeg, n, true, aside->stream))) return s;
      MG_HIP (hipEventRecord (aside->done, aside->stream));
      aside->launched = true;
    }
  return MG_OK;
}
