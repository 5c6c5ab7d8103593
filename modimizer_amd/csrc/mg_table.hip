/* mg_table.hip — K3/K4/K5: the device-resident modset table for gfx950.
 *
 * What it must reproduce (reference modset.c:45-62 and its callers): looking a k-mer up returns
 * its index or 0; inserting a new k-mer gives it index ++max, i.e. indices are handed out in
 * order of FIRST OCCURRENCE in the (read,pos)-ordered modimizer stream, and every occurrence bumps
 * a saturating 16-bit depth (modutils.c:26).
 *
 * Layout.  The device table is not the reference's index[] array (with a power-of-two modulus d
 * every primary slot of that table has its low log2(d) bits zero, because the hash that picks the
 * slot is the hash that was just tested to be 0 mod d; that layout is only materialised on
 * request by mgReplayIndexKernel).  Here: NB buckets of R slots of 16 bytes {mix(kmer)+1, ord, cnt},
 * where mix is a bijection of the 2k-bit k-mers (mgMixK); a k-mer's bucket is the top bits of its mixed
 * value, its home slot the low bits, and linear probing wraps INSIDE the bucket, so a bucket is a
 * self-contained little table that fits LDS.
 * ord: 0 = none, bit 31 set = assigned index, otherwise a transient first-occurrence token.
 *
 * Two build paths, same table, same results:
 *
 *  direct   (small batches)  global atomics: CAS the key in, post a token that is larger the
 *           earlier the occurrence (atomicMax: assigned indices have bit 31 set, so they are never
 *           lowered), atomicAdd the count; then a streaming pass asks every occurrence "is the
 *           slot's token mine?" - exactly the first occurrences say yes - and an ordered count
 *           over those flags turns them into max+1, max+2, ...
 *
 *  bucketed (large batches)  no global atomics on the data path.  Measured on MI355X: a random
 *           global atomic costs ~1/17 G/s (three on one slot serialise), a random load ~1/45 G/s,
 *           streaming ~5 TB/s.  So: (1) radix-partition the batch by bucket (two streaming passes; the
 *           first reads the scan's per-worker segments as they are, MgSegSrc, and its digit counts come
 *           from the scan kernel), (2) one workgroup per bucket dedups its occurrences in LDS (LDS
 *           atomics), flags the first occurrence of every k-mer that is new to the table (or clears the
 *           flags of the others: markDup) and writes the bucket's unique k-mers back grouped by the slice
 *           of the ordinal range their first occurrence lies in, (3) an ordered count over the flags gives
 *           every new k-mer its index, writes value[] in order and leaves a rank record per 64 ordinals,
 *           (3b) the rank lookups turn the uniques' ordinals into indices slice by slice, an XCD reading
 *           one slice's rank records from its own L2, (4) one workgroup per bucket merges the bucket's
 *           unique k-mers into its LDS copy of the table bucket and streams it back.
 *
 * Files.  Here: the partition's element format and the table's life cycle -- geometry, allocation and lazy zeroing, rehash and rollback,
 * the loader, the layout check.  mgTableAdd -- the direct path's kernels, the plan (mgAddPlan), the scratch, the launches -- is
 * mg_tableadd.hip; the ordered flag count and index assignment of both paths (step 3, and the prune's) is mg_rank.hip; step 1 is
 * mg_part.hip, steps 2, 3b and 4 are mg_bucket.hip; every lookup is mg_find.hip; the passes over a whole set (export, histogram, index
 * replay, merge, prune) are mg_tableset.hip.  What they share is mg_table.h (internal to these files).  A kernel is defined, launched
 * and given its attributes in one file only.
 */
#include "mg_table.h"

static inline int mgLog2 (U64 x) { int l = 0; while (((U64) 1 << l) < x) ++l; return l; }

/* the element format of the partition passes for a batch of n whose first pass sorts by the top hiB bits of the bucket id, and whether
   an element then fits one packed 8-byte word: the mixed k-mer without its coarse digit and the ordinal in 64 bits */
MgPartFmt mgPartFmtOf (const MgTable *t, U64 n, int hiB)
{ MgPartFmt f; f.ordBits = mgLog2 (n) > 1 ? mgLog2 (n) : 1; f.remBits = t->kbits - hiB; f.loB = t->log2NB - hiB; return f; }
bool mgPartFmtFits (const MgTable *t, const MgPartFmt &f) { return t->kbits >= t->log2NB + 4 && f.remBits + f.ordBits <= 64; }

/* ======================================================================================== */
/* table life cycle: allocation, lazy zeroing, growth                                         */

/* the overflow flag (counters[1]) comes back through the table's page-locked words, or by a plain copy where it has none */
static MgStatus mgReadOverflow (MgTable *t, hipStream_t st, U64 *over)
{
  if (t->pin)
    { MG_HIP (hipMemcpyAsync (t->pin + 3, t->counters + 1, 8, hipMemcpyDeviceToHost, st));
      MG_HIP (hipStreamSynchronize (st));
      *over = t->pin[3];
    }
  else
    { MG_HIP (hipStreamSynchronize (st));
      MG_HIP (hipMemcpy (over, t->counters + 1, 8, hipMemcpyDeviceToHost));
    }
  return MG_OK;
}

/* zero the buckets nothing has been written to (occ == 0); everything else is left alone */
__global__ __launch_bounds__ (256)
void mgCleanEmptyBucketsKernel (MgSlot *__restrict__ slots, MgGeom g, const U32 *__restrict__ occ, U32 nBuckets)
{
  const uint4 z = make_uint4 (0, 0, 0, 0);
  for (U32 b = blockIdx.x ; b < nBuckets ; b += gridDim.x)
    { if (occ[b]) continue;
      for (U32 i = threadIdx.x ; i < g.R ; i += blockDim.x) *reinterpret_cast<uint4 *> (&slots[(U64) b * g.R + i]) = z;
    }
}

/* old table -> new table (another geometry): every assigned entry is re-inserted with its index and count */
__global__ void mgRehashKernel (const MgSlot *__restrict__ oldSlots, U32 oldNB, const U32 *__restrict__ oldOcc, U32 oldR,
                                MgSlot *__restrict__ slots, MgGeom g, U32 *__restrict__ occ, U64 *counters, U32 keepMax)
{
  for (U32 bk = blockIdx.x ; bk < oldNB ; bk += gridDim.x)
    { if (!oldOcc[bk]) continue;
      const MgSlot *from = oldSlots + (U64) bk * oldR;
      for (U32 i = threadIdx.x ; i < oldR ; i += blockDim.x)
        { uint4 v = *reinterpret_cast<const uint4 *> (&from[i]);
          if (!mgLiveEntry (v, keepMax)) continue;      /* (keepMax: what a refused add left behind is dropped, mgTableRollback) */
          const unsigned long long key = mgKeyOf (v);
          const U64 m = key - 1;                                  /* the key IS the mixed k-mer: no re-hash needed to re-place it */
          const U32 b = mgBucketOfM (m, g);
          const U64 base = (U64) b * g.R;
          U32 at = mgHomeOfM (m, g);
          bool placed = false;
          for (U32 probes = 0 ; probes < g.R ; ++probes)
            { if (slots[base + at].key == 0 && atomicCAS ((unsigned long long *) &slots[base + at].key, 0ull, key) == 0) { placed = true; break; }
              at = mgNextSlot (at, g.R);
            }
          if (!placed) { counters[1] = 1; continue; }
          slots[base + at].ord = v.z; slots[base + at].cnt = v.w;
          if (!occ[b]) occ[b] = 1;
        }
    }
}

/* The same bucket by bucket (round 6): a bucket is a self-contained table and its id a prefix of its keys, so when NB stays or grows a NEW bucket's
   entries all come from ONE old bucket (its id's leading bits).  A workgroup per new bucket reads the parent's slots as a stream, claims the entries
   that are its own in an LDS image of the new geometry and streams the image out: no global atomic, every byte read and written once or twice
   (tools/incremental_probe.py: 4.4 -> 1.3 ms for 9.3e7 entries). */
__global__ __launch_bounds__ (1024)
void mgRehashBucketKernel (const MgSlot *__restrict__ oldSlots, int oldLog2NB, const U32 *__restrict__ oldOcc, U32 oldR,
                           MgSlot *__restrict__ slots, MgGeom g, U32 *__restrict__ occ, U64 *counters, U32 keepMax)
{
  unsigned long long *sKey = reinterpret_cast<unsigned long long *> (mgDynLds);
  U32 *sOrd = reinterpret_cast<U32 *> (mgDynLds + (size_t) g.R * 8);
  U32 *sCnt = sOrd + g.R;
  U32 *sN = sCnt + g.R;
  const U32 T = blockDim.x, tid = threadIdx.x, NB = 1u << g.log2NB;
  const int up = g.log2NB - oldLog2NB;                                /* >= 0 */
  for (U32 b = blockIdx.x ; b < NB ; b += gridDim.x)
    { const U32 parent = b >> up;
      if (!oldOcc[parent]) continue;                                  /* (uniform) nothing there: the new bucket stays unwritten, occ 0 */
      for (U32 i = tid ; i < g.R ; i += T) { sKey[i] = 0; sOrd[i] = 0; sCnt[i] = 0; }
      if (tid == 0) sN[0] = 0;
      __syncthreads ();
      const MgSlot *from = oldSlots + (U64) parent * oldR;
      U32 mine = 0;
      for (U32 i = tid ; i < oldR ; i += T)
        { const uint4 v = *reinterpret_cast<const uint4 *> (&from[i]);
          if (!mgLiveEntry (v, keepMax)) continue;
          const unsigned long long key = mgKeyOf (v);
          const U64 m = key - 1;
          if (mgBucketOfM (m, g) != b) continue;
          const U32 at = mgLdsClaim (sKey, g.R, mgHomeOfM (m, g), key);
          if (at == g.R) { counters[1] = 1; continue; }
          sOrd[at] = v.z; sCnt[at] = v.w; ++mine;
        }
      if (mine) atomicAdd (&sN[0], mine);
      __syncthreads ();
      const U32 n = sN[0];
      if (n)                                                          /* (uniform) */
        { for (U32 i = tid ; i < g.R ; i += T)
            { const unsigned long long k = sKey[i];
              typedef unsigned v4u __attribute__ ((ext_vector_type (4)));
              v4u vv = { (U32) k, (U32) (k >> 32), sOrd[i], sCnt[i] };
              __builtin_nontemporal_store (vv, reinterpret_cast<v4u *> (&slots[(U64) b * g.R + i]));
            }
          if (tid == 0) occ[b] = n;
        }
      __syncthreads ();
    }
}

#define MG_FINE_LOG2 18            /* the most buckets a table has (mgSetGeometry): counts per finest bucket give every coarser geometry's by addition */
/* How many entries every bucket of the finest geometry (2^MG_FINE_LOG2 buckets) would hold: a bucket id is a prefix of the key, so the
   counts of any coarser geometry are sums of these.  From the table's assigned entries, or from value[first .. last]. */
__global__ void mgFineCountSlotsKernel (const MgSlot *__restrict__ slots, U32 NB, const U32 *__restrict__ occ, U32 R, int kbits, U32 keepMax, U32 *__restrict__ fine)
{
  MgGeom g; g.R = R; g.log2NB = MG_FINE_LOG2 < kbits ? MG_FINE_LOG2 : kbits; g.kbits = kbits;
  for (U32 bk = blockIdx.x ; bk < NB ; bk += gridDim.x)
    { if (!occ[bk]) continue;                                      /* (never written: its bytes are undefined) */
      for (U32 i = threadIdx.x ; i < R ; i += blockDim.x)
        { const uint4 v = *reinterpret_cast<const uint4 *> (&slots[(U64) bk * R + i]);
          if (!mgLiveEntry (v, keepMax)) continue;
          const U64 m = (mgKeyOf (v) - 1) & (kbits >= 64 ? ~0ull : (((U64) 1 << kbits) - 1));
          atomicAdd (&fine[mgBucketOfM (m, g)], 1u);               /* (m < 2^kbits: the id is below 2^log2NB) */
        }
    }
}
__global__ void mgFineCountValuesKernel (const U64 *__restrict__ value, U32 first, U32 last, int kbits, U32 *__restrict__ fine)
{
  MgGeom g; g.R = MG_R_QUANTUM; g.log2NB = MG_FINE_LOG2 < kbits ? MG_FINE_LOG2 : kbits; g.kbits = kbits;
  const U64 mask = kbits >= 64 ? ~0ull : (((U64) 1 << kbits) - 1);
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for (U64 i = (U64) first + (U64) blockIdx.x * blockDim.x + threadIdx.x ; i <= last ; i += stride)
    atomicAdd (&fine[mgBucketOfM (mgMixK (value[i] & mask, kbits) & mask, g)], 1u);
}

/* Geometry for `want` slots: NB a power of two, R = want / NB rounded up to a multiple of 64, between half of wantR and wantR where the size
   allows (R = 4096: a bucket's image is 64 KiB of LDS); at most 2^18 buckets (two 9-bit partition passes), R up to 8192 beyond that. */
static U32 mgOwnR (const MgTable *t)               /* the table's own limit on R: wantR (0: 4096) within what the kernels take */
{
  U32 R = t->wantR ? t->wantR : 4096;
  if (R > 8192) R = 8192;                         /* the dedup kernel's threads hold MG_DEDUP_PER (R <= 4096) or MG_DEDUP_PER_BIG slots each */
  if (R < MG_R_QUANTUM) R = MG_R_QUANTUM;
  return R;
}
static void mgSetGeometry (MgTable *t, U64 want)
{
  const U32 Rmax = mgOwnR (t);
  if (want < MG_R_QUANTUM) want = MG_R_QUANTUM;
  int lgNB = 0;
  while (lgNB < 18 && (want + ((U64) 1 << lgNB) - 1) / ((U64) 1 << lgNB) > Rmax) ++lgNB;
  U64 R = (want + ((U64) 1 << lgNB) - 1) >> lgNB;
  R = (R + MG_R_QUANTUM - 1) / MG_R_QUANTUM * MG_R_QUANTUM;
  if (R > 8192) R = 8192;
  mgTableSetGeom (t, lgNB, (U32) R);
}

/* The smallest legal geometry of at least `want` slots whose fullest bucket holds its entries with one slot to spare (a bucket that is
   offered as many keys as it has slots refuses them: mgBucketMergeKernel), from the fine counts.  Legal: NB a power of two up to 2^18,
   R a multiple of 64 up to the table's own limit (wantR) -- or, where nothing else fits, up to 8192 -- and no more slots than the set's
   table bits allow (maxLog2Slots).  MG_ERR_CAPACITY when there is none. */
static MgStatus mgFitGeometry (const MgTable *t, const U32 *dFine, U64 want, int *lgOut, U32 *ROut, hipStream_t st)
{
  const size_t nFine = (size_t) 1 << MG_FINE_LOG2;
  U32 *h = (U32 *) malloc (nFine * sizeof (U32));
  if (!h) { mgSetError ("out of host memory"); return MG_ERR_NOMEM; }
  if (hipMemcpyAsync (h, dFine, nFine * sizeof (U32), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess)
    { free (h); return mgHipFail (hipGetLastError (), "mgFitGeometry"); }
  const int fineLg = MG_FINE_LOG2 < t->kbits ? MG_FINE_LOG2 : t->kbits;
  U64 fullest[MG_FINE_LOG2 + 1];
  for (int lg = fineLg ; lg >= 0 ; --lg)
    { U32 m = 0;
      for (size_t i = 0 ; i < ((size_t) 1 << lg) ; ++i) if (h[i] > m) m = h[i];
      fullest[lg] = m;
      if (lg) for (size_t i = 0 ; i < ((size_t) 1 << (lg - 1)) ; ++i) h[i] = h[2 * i] + h[2 * i + 1];
    }
  free (h);
  if (want < MG_R_QUANTUM) want = MG_R_QUANTUM;
  const U32 limits[2] = { mgOwnR (t), 8192 };
  /* the most slots a geometry may have: what the table bits allow -- or what mgSetGeometry makes of `want` itself, which rounds R up */
  U64 maxSlots = (U64) 1 << t->maxLog2Slots;
  { MgTable byMean = *t; mgSetGeometry (&byMean, want); if (byMean.nSlots > maxSlots) maxSlots = byMean.nSlots; }
  for (int pass = 0 ; pass < 2 ; ++pass)
    { U64 best = 0;
      for (int lg = 0 ; lg <= fineLg ; ++lg)
        { U64 R = (want + ((U64) 1 << lg) - 1) >> lg;
          if (R < fullest[lg] + 1) R = fullest[lg] + 1;
          R = (R + MG_R_QUANTUM - 1) / MG_R_QUANTUM * MG_R_QUANTUM;
          if (R > limits[pass]) continue;
          const U64 slots = R << lg;
          if (slots > maxSlots) continue;
          if (!best || slots < best) { best = slots; *lgOut = lg; *ROut = (U32) R; }
        }
      if (best) return MG_OK;
    }
  mgSetError ("no geometry of the device table holds the set: its fullest bucket has %llu entries in 2^%d buckets (at most 8192 slots a bucket, 2^%d slots)",
              (unsigned long long) fullest[fineLg], fineLg, t->maxLog2Slots);
  return MG_ERR_CAPACITY;
}

/* The same from the counts that count (dFine) leaves: one of the two fine-count kernels, launched on st over the zeroed array of
   2^MG_FINE_LOG2 words that is handed to it.  The array lives as long as this call, on every path. */
template <class F> static MgStatus mgFitByFineCounts (const MgTable *t, U64 want, int *lgOut, U32 *ROut, hipStream_t st, F count)
{
  U32 *dFine = 0;
  if (hipMalloc ((void **) &dFine, sizeof (U32) << MG_FINE_LOG2) != hipSuccess) return mgHipFail (hipGetLastError (), "hipMalloc");
  MgStatus s;
  if (hipMemsetAsync (dFine, 0, sizeof (U32) << MG_FINE_LOG2, st) != hipSuccess) s = mgHipFail (hipGetLastError (), "hipMemsetAsync");
  else { count (dFine); s = mgFitGeometry (t, dFine, want, lgOut, ROut, st); }
  (void) hipFree (dFine);
  return s;
}

/* an empty table of the geometry t names (R, log2NB, nSlots); memory is only allocated when the capacity is short */
static MgStatus mgTableAllocGeom (MgTable *t, hipStream_t st)
{
  const U32 NB = (U32) 1 << t->log2NB;
  if (!t->slots || t->nSlots > t->capSlots)
    { if (t->slots) { MG_HIP (hipStreamSynchronize (st)); MG_HIP (hipFree (t->slots)); t->slots = 0; t->capSlots = 0; }
      MG_HIP (hipMalloc ((void **) &t->slots, t->nSlots * sizeof (MgSlot)));
      t->capSlots = t->nSlots;
    }
  if (!t->occ || NB > t->capNB)
    { if (t->occ) { MG_HIP (hipStreamSynchronize (st)); MG_HIP (hipFree (t->occ)); t->occ = 0; t->capNB = 0; }
      MG_HIP (hipMalloc ((void **) &t->occ, (size_t) NB * sizeof (U32)));
      t->capNB = NB;
    }
  mgTableForget (t, st);
  return MG_OK;
}

/* the same of (at least) `want` slots */
MgStatus mgTableAlloc (MgTable *t, U64 want, hipStream_t st)
{
  mgSetGeometry (t, want);
  return mgTableAllocGeom (t, st);
}

void mgTableForget (MgTable *t, hipStream_t st)
{
  (void) hipMemsetAsync (t->occ, 0, ((size_t) 1 << t->log2NB) * sizeof (U32), st);
  t->dirty = true;               /* no memset of the slots: a bucket is defined once something wrote all of it */
  t->liveHistValid = false;
  t->empty = true; ++t->version;
}

MgStatus mgTableClean (MgTable *t, hipStream_t st)
{
  if (!t->dirty) return MG_OK;
  U32 NB = (U32) 1 << t->log2NB;
  MG_LAUNCH (MG_K_MEMSET, st, mgCleanEmptyBucketsKernel, dim3 (NB < 4096 ? NB : 4096), dim3 (256), 0, st, t->slots, mgGeomOf (t), t->occ, NB);
  MG_HIP (hipGetLastError ());
  t->dirty = false;
  return MG_OK;
}

/* slots needed so that `entries` fit at the table's load (0.6 unless the caller set loadPct); at most 2^maxLog2Slots */
static U64 mgSlotsFor (const MgTable *t, U64 entries)
{
  const long lk = mgKnobs ()->tableLoad;
  const int envPct = lk != MG_KNOB_UNSET && lk >= 10 && lk <= 150 ? (int) lk : 0;   /* dev knob (above 100: experiments only) */
  const int loadPct = envPct ? envPct : (t->loadPct ? t->loadPct : 60);
  U64 need = entries * 100 / (U64) loadPct + 1;      /* entries / 0.6 by default */
  if (need < ((U64) 1 << 16)) need = (U64) 1 << 16;
  if (need > ((U64) 1 << t->maxLog2Slots)) need = (U64) 1 << t->maxLog2Slots;
  return need;
}

/* The table in another geometry: the assigned entries re-placed (their keys are their hashes).  The new geometry is sized by the MEAN
   bucket (mgSetGeometry), and a set whose keys crowd one bucket may not fit it: the kernels raise the overflow flag, which is read here,
   before anything zeroes it.  Then the old table -- kept until the new one is complete -- is counted by finest bucket, the smallest legal
   geometry that holds its fullest bucket is taken (mgFitGeometry), and the entries are placed again.  MG_ERR_CAPACITY only when no legal
   geometry holds them; the old table is then still in place and still answers.
   exact: that geometry (log2NB, R) instead of one for `want` slots.  keepMax: entries with a larger index are dropped (mgTableRollback). */
struct MgOldTable { MgSlot *slots; U32 *occ; U64 nSlots, capSlots; U32 capNB, R; int log2NB; bool dirty; };
static void mgTableTakeOld (MgTable *t, MgOldTable *o)
{ o->slots = t->slots; o->occ = t->occ; o->nSlots = t->nSlots; o->capSlots = t->capSlots; o->capNB = t->capNB; o->R = t->R; o->log2NB = t->log2NB; o->dirty = t->dirty;
  t->slots = 0; t->occ = 0; t->capSlots = 0; t->capNB = 0; }
static void mgTablePutOld (MgTable *t, const MgOldTable &o, hipStream_t st)
{ (void) hipStreamSynchronize (st);
  if (t->slots) (void) hipFree (t->slots);
  if (t->occ) (void) hipFree (t->occ);
  t->slots = o.slots; t->occ = o.occ; t->nSlots = o.nSlots; t->capSlots = o.capSlots; t->capNB = o.capNB; t->R = o.R; t->log2NB = o.log2NB; t->dirty = o.dirty;
  t->empty = false; ++t->version; }

/* one pass old -> t (allocated, every occ[] zero), waited for; *over != 0: a new bucket had no room */
static MgStatus mgRehashPass (MgTable *t, const MgOldTable &o, U32 keepMax, hipStream_t st, U64 *over)
{
  MgStatus s;
  const U32 oldNB = (U32) 1 << o.log2NB;
  MG_HIP (hipMemsetAsync (t->counters + 1, 0, 8, st));
  if (t->log2NB >= o.log2NB && mgKnobs ()->tablePath != 'd')             /* bucket by bucket, out of LDS (the new buckets nothing goes into stay unwritten: dirty again) */
    { const U32 NB = (U32) 1 << t->log2NB;
      const size_t lds = (size_t) t->R * 16 + 16;
      if (lds > 48 * 1024) MG_HIP (hipFuncSetAttribute ((const void *) mgRehashBucketKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
      MG_HIP (hipMemsetAsync (t->occ, 0, (size_t) NB * sizeof (U32), st));
      ++t->diag[MG_DIAG_REHASH_BUCKET];
      MG_LAUNCH (MG_K_TABLE_LOAD, st, mgRehashBucketKernel, dim3 (NB < 2048 ? NB : 2048), dim3 (1024), lds, st,
                 o.slots, o.log2NB, o.occ, o.R, t->slots, mgGeomOf (t), t->occ, t->counters, keepMax);
      t->dirty = true;
    }
  else
    { if ((s = mgTableClean (t, st))) return s;                          /* (the atomic path claims slots in a zeroed table) */
      ++t->diag[MG_DIAG_REHASH_ATOMIC];
      MG_LAUNCH (MG_K_TABLE_LOAD, st, mgRehashKernel, dim3 (oldNB < 8192 ? oldNB : 8192), dim3 (256), 0, st,
                 o.slots, oldNB, o.occ, o.R, t->slots, mgGeomOf (t), t->occ, t->counters, keepMax);
    }
  MG_HIP (hipGetLastError ());
  return mgReadOverflow (t, st, over);
}

static MgStatus mgTableRehash (MgTable *t, U64 want, bool exact, int exactLg, U32 exactR, U32 keepMax, hipStream_t st)
{
  MgOldTable o; mgTableTakeOld (t, &o);
  MgStatus s = MG_OK;
  for (int attempt = 0 ; attempt < 2 ; ++attempt)
    { if (attempt == 0 && exact) mgTableSetGeom (t, exactLg, exactR);
      else if (attempt == 0) mgSetGeometry (t, want);
      else
        { int lg = 0; U32 R = 0;
          const U32 oldNB = (U32) 1 << o.log2NB;
          s = mgFitByFineCounts (t, want, &lg, &R, st, [&] (U32 *dFine)
            { MG_LAUNCH (MG_K_TABLE_HIST, st, mgFineCountSlotsKernel, dim3 (oldNB < 8192 ? oldNB : 8192), dim3 (256), 0, st, o.slots, oldNB, o.occ, o.R, t->kbits, keepMax, dFine); });
          if (s) break;
          mgTableSetGeom (t, lg, R);
        }
      if ((s = mgTableAllocGeom (t, st))) break;
      U64 over = 0;
      if ((s = mgRehashPass (t, o, keepMax, st, &over))) break;
      if (!over)
        { MG_HIP (hipFree (o.slots)); MG_HIP (hipFree (o.occ));
          t->empty = false; ++t->version;
          return MG_OK;
        }
      (void) hipFree (t->slots); (void) hipFree (t->occ);
      t->slots = 0; t->occ = 0; t->capSlots = 0; t->capNB = 0;
      if (attempt) { mgSetError ("internal: the device table's fitted geometry (2^%d x %u) does not hold its entries", t->log2NB, t->R); s = MG_ERR_CAPACITY; }
    }
  mgTablePutOld (t, o, st);
  return s;
}
static MgStatus mgTableRehashTo (MgTable *t, U64 want, hipStream_t st) { return mgTableRehash (t, want, false, 0, 0, 0x7fffffffu, st); }
static MgStatus mgTableRehashExact (MgTable *t, int log2NB, U32 R, hipStream_t st) { return mgTableRehash (t, (U64) R << log2NB, true, log2NB, R, 0x7fffffffu, st); }

/* After an add that was refused (MG_ERR_CAPACITY: the set's size reached, or a bucket without room) the table holds what the add had
   written by then: keys without an index, and entries whose index lies beyond max.  They go, by a pass over the table that keeps the
   entries 1 .. max: the set then answers as before the add, on every lookup path.  The pass is a whole rehash into a second allocation of
   the table's size: the price of an error the reference program exits on.  Where that allocation fails the caller gets MG_ERR_HIP in the
   place of MG_ERR_CAPACITY, and the table keeps what the add wrote (the old table is put back as it was).  Depth counts the refused batch
   had added to earlier entries stay: they are not the table's to take back. */
MgStatus mgTableRollback (MgTable *t, hipStream_t st)
{
  t->liveHistValid = false;
  if (!t->slots) return MG_OK;
  return mgTableRehash (t, t->nSlots, true, t->log2NB, t->R, t->max, st);
}

MgStatus mgTableEnsure (MgTable *t, U64 nIncoming, hipStream_t st)
{
  U64 want = mgSlotsFor (t, (U64) t->max + nIncoming);
  if (t->slots && want <= t->nSlots) return MG_OK;
  if (!t->slots || !t->max) return mgTableAlloc (t, want, st);
  /* grow: a table that takes adds doubles at least (sized to the entry, every add would re-place everything; doubling re-places every
     entry twice over a set's life, growing by half three times: tools/incremental_probe.py, ten 1 Gbp batches into one set, 34.9 against 30 ms) */
  if (nIncoming && want < 2 * t->nSlots) want = 2 * t->nSlots;
  if (want > ((U64) 1 << t->maxLog2Slots)) want = (U64) 1 << t->maxLog2Slots;
  if (want <= t->nSlots) return MG_OK;
  return mgTableRehashTo (t, want, st);
}

/* ======================================================================================== */
/* the layout check                                                                           */

/* A check of the table's layout that does not go through the lookups: a thread per slot walks from its key's home to the slot.
   out[0] += keys whose walk crosses an empty slot (a lookup would stop there), out[1] += keys in a bucket other than the one they
   imply, out[2] += keys met a second time on that walk (a duplicate inside the bucket), out[3] += keys */
__global__ __launch_bounds__ (256)
void mgTableCheckLayoutKernel (const MgSlot *__restrict__ slots, MgGeom g, U64 nSlots, unsigned long long *__restrict__ out)
{
  const U64 stride = (U64) gridDim.x * blockDim.x;
  U32 broken = 0, stray = 0, dup = 0, keys = 0;
  for (U64 o = (U64) blockIdx.x * blockDim.x + threadIdx.x ; o < nSlots ; o += stride)
    { const uint4 v = *reinterpret_cast<const uint4 *> (&slots[o]);
      const U64 key = mgKeyOf (v);
      if (!key) continue;
      ++keys;
      const U32 bkt = (U32) (o / g.R), me = (U32) (o - (U64) bkt * g.R);
      const U64 m = key - 1;
      if (mgBucketOfM (m, g) != bkt) { ++stray; continue; }
      const U64 base = (U64) bkt * g.R;
      for (U32 at = mgHomeOfM (m, g) ; at != me ; at = mgNextSlot (at, g.R))
        { const uint4 w = *reinterpret_cast<const uint4 *> (&slots[base + at]);
          const U64 k2 = mgKeyOf (w);
          if (!k2) { ++broken; break; }
          if (k2 == key) { ++dup; break; }
        }
    }
  if (broken) atomicAdd (&out[0], (unsigned long long) broken);
  if (stray) atomicAdd (&out[1], (unsigned long long) stray);
  if (dup) atomicAdd (&out[2], (unsigned long long) dup);
  if (keys) atomicAdd (&out[3], (unsigned long long) keys);
}

/* dOut: four device words (see the kernel), zeroed here */
MgStatus mgTableLayoutCheck (MgTable *t, U64 *dOut, hipStream_t st)
{
  { MgStatus cs = mgTableClean (t, st); if (cs) return cs; }
  MG_HIP (hipMemsetAsync (dOut, 0, 32, st));
  MG_LAUNCH (MG_K_TABLE_FIND, st, mgTableCheckLayoutKernel, dim3 (mgGridWide (t->nSlots)), dim3 (256), 0, st, t->slots, mgGeomOf (t), t->nSlots, (unsigned long long *) dOut);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

/* ======================================================================================== */
/* the loader                                                                                 */

/* entries first..last (with their existing indices) from a host modset into the device table */
__global__ void mgTableLoadKernel (MgSlot *__restrict__ slots, MgGeom g, const U64 *__restrict__ value,
                                   U32 first, U32 last, U32 *__restrict__ occ, U64 *counters)
{
  U64 i = (U64) first + (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; i <= last ; i += stride)
    { const U64 m = mgMixK (value[i], g.kbits), key = m + 1;
      const U32 b = mgBucketOfM (m, g);
      const U64 base = (U64) b * g.R;
      U32 at = mgHomeOfM (m, g);
      bool placed = false, dup = false;
      for (U32 probes = 0 ; probes < g.R ; ++probes)
        { U64 cur = slots[base + at].key;
          if (cur == 0)
            { cur = atomicCAS ((unsigned long long *) &slots[base + at].key, 0ull, (unsigned long long) key);
              if (cur == 0) { placed = true; break; }
            }
          if (cur == key) { dup = true; break; }     /* duplicate value in the host arrays: keep the first */
          at = mgNextSlot (at, g.R);
        }
      if (placed) { slots[base + at].ord = (U32) i | MG_ASSIGNED; atomicAdd (&occ[b], 1u); }
      else if (!dup) counters[1] = 1;
    }
}

/* the loader, waited for; *over != 0: a bucket had no room for one of the values (the others are in) */
static MgStatus mgLoadLaunch (MgTable *t, const U64 *dValue, U32 first, U32 last, hipStream_t st, U64 *over)
{
  MG_HIP (hipMemsetAsync (t->counters + 1, 0, 8, st));
  MG_LAUNCH (MG_K_TABLE_LOAD, st, mgTableLoadKernel, dim3 (mgGridWide ((U64) last - first + 1)), dim3 (256), 0, st,
             t->slots, mgGeomOf (t), dValue, first, last, t->occ, t->counters);
  MG_HIP (hipGetLastError ());
  return mgReadOverflow (t, st, over);
}

MgStatus mgTableLoadHost (MgTable *t, const U64 *dValue, U32 first, U32 last, hipStream_t st)
{
  if (last < first) return MG_OK;
  t->liveHistValid = false; t->empty = false; ++t->version;
  { MgStatus cs = mgTableClean (t, st); if (cs) return cs; }
  U64 over = 0;
  MgStatus s = mgLoadLaunch (t, dValue, first, last, st, &over);
  if (s || !over) return s;
  /* A bucket had no room: the table was sized by the mean (mgTableEnsure) and these values crowd one bucket.  The entries that found
     a slot stay where they are; the table goes into a geometry that holds the fullest bucket of ALL the values (value[1 .. last]:
     what is in the table and what was left out), and the values are loaded again -- those already there are met as duplicates. */
  int lg = 0; U32 R = 0;
  s = mgFitByFineCounts (t, mgSlotsFor (t, last), &lg, &R, st, [&] (U32 *dFine)
    { MG_LAUNCH (MG_K_TABLE_HIST, st, mgFineCountValuesKernel, dim3 (mgGridWide (last)), dim3 (256), 0, st, dValue, 1u, last, t->kbits, dFine); });
  if (!s) s = mgTableRehashExact (t, lg, R, st);
  if (s) return s;
  if ((s = mgLoadLaunch (t, dValue, first, last, st, &over))) return s;
  if (over) { mgSetError ("internal: the device table's fitted geometry (2^%d x %u) does not hold the host's entries", lg, R); return MG_ERR_CAPACITY; }
  return MG_OK;
}
