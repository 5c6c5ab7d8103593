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
 * Files.  Here: the direct build, the ordered flag count and index assignment of both paths, the table's life cycle (geometry,
 * clean, rehash, load), mgTableAdd -- plan (mgAddPlan), carve, launches -- and the whole-set passes.  Step 1 is mg_part.hip, steps 2,
 * 3b and 4 are mg_bucket.hip, every lookup is mg_find.hip; what they share is mg_table.h (internal to these files).  A kernel is
 * defined, launched and given its attributes in one file only.
 */
#include <atomic>
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

/* Ordered count of first-occurrence flags.  The ordinal range is cut into contiguous pieces, one
 * per wave ("rank unit"); a wave walks its piece in rows of 64 ordinals, so flags, k-mers and the
 * value[] it writes are all lane-contiguous.  Pass A counts per unit, a one-block scan turns the
 * counts into bases, pass B assigns. */

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


__global__ __launch_bounds__ (256)
void mgRankCountKernel (const unsigned char *__restrict__ flags, U64 n, U64 rowsPerUnit, U64 *__restrict__ unitCount)
{
  MG_BUILD_PRIO ();
  const int lane = threadIdx.x & 63;
  const U64 unit = (U64) blockIdx.x * 4 + (threadIdx.x >> 6);
  const U64 nRows = (n + 63) / 64;
  U64 row = unit * rowsPerUnit, rEnd = row + rowsPerUnit;
  if (rEnd > nRows) rEnd = nRows;
  U32 c = 0;
  /* a lane reads 16 consecutive flags at once (one 16-byte load: a wave covers 16 rows), four such loads in flight */
  if ((reinterpret_cast<uintptr_t> (flags) & 15) == 0)
    for ( ; row + 64 <= rEnd && (row + 64) * 64 <= n ; row += 64)
      { uint4 q[4];
#pragma unroll
        for (int j = 0 ; j < 4 ; ++j) q[j] = *reinterpret_cast<const uint4 *> (flags + (row + 16 * j) * 64 + (U64) lane * 16);
#pragma unroll
        for (int j = 0 ; j < 4 ; ++j)
          c += (U32) __popc (q[j].x & 0x01010101u) + (U32) __popc (q[j].y & 0x01010101u) + (U32) __popc (q[j].z & 0x01010101u) + (U32) __popc (q[j].w & 0x01010101u);
      }
  for ( ; row + 4 <= rEnd ; row += 4)
    { U32 v[4];
#pragma unroll
      for (int j = 0 ; j < 4 ; ++j) { U64 o = (row + j) * 64 + lane; v[j] = (o < n) ? (flags[o] & 1) : 0; }
      c += v[0] + v[1] + v[2] + v[3];
    }
  for ( ; row < rEnd ; ++row) { U64 o = row * 64 + lane; c += (o < n) ? (flags[o] & 1) : 0; }
  c = mgWaveReduce<MgSum> (c);
  if (lane == 0) unitCount[unit] = c;
}

/* pass B: every flagged ordinal o gets index baseMax+1+rank(o); value[index] = kmer[o].
 * DIRECT: also store the index in the slot.  Otherwise (mgTablePrune): record, per row of 64 ordinals, the flag
 * bitmap and the number of flags before the row, for the pass that moves the survivors' depths.
 * The bucketed leg of mgTableAdd does the two halves apart: mgRankRecordKernel, then mgValueWriteKernel. */
#define MG_RANK_ROWS 8
template <bool DIRECT>
__global__ __launch_bounds__ (256)
void mgRankAssignKernel (const unsigned char *__restrict__ flags, const U64 *__restrict__ kmer,
                         U64 n, U64 rowsPerUnit,
                         const U64 *__restrict__ unitBase, U32 baseMax, U32 size,
                         U64 *__restrict__ value, MgSlot *__restrict__ slots, const U32 *__restrict__ slotId,
                         MgRankGrp *__restrict__ grp)
{
  MG_BUILD_PRIO ();
  const int lane = threadIdx.x & 63;
  const U64 unit = (U64) blockIdx.x * 4 + (U32) __builtin_amdgcn_readfirstlane ((int) (threadIdx.x >> 6));
  const U64 nRows = (n + 63) / 64;
  U64 row = unit * rowsPerUnit, rEnd = row + rowsPerUnit;
  if (rEnd > nRows) rEnd = nRows;
  if (row >= rEnd) return;
  U64 run = unitBase[unit];
  const U64 below = ((U64) 1 << lane) - 1;
  /* MG_RANK_ROWS rows per step: the loads of all of them are in flight before the first ballot */
  for ( ; row < rEnd ; row += MG_RANK_ROWS)
    { bool f[MG_RANK_ROWS]; U64 km[MG_RANK_ROWS]; U32 fl[MG_RANK_ROWS];
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j)
        { const U64 o = (row + j) * 64 + lane;
          const bool in = (row + j < rEnd) && (o < n);
          fl[j] = flags[in ? o : 0];
        }
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j)
        { const U64 o = (row + j) * 64 + lane;
          const bool in = (row + j < rEnd) && (o < n);
          km[j] = in ? __builtin_nontemporal_load (&kmer[o]) : 0;
        }
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j)
        { const U64 o = (row + j) * 64 + lane;
          f[j] = (row + j < rEnd) && (o < n) && (fl[j] & 1);
          /* every load has landed before the first store goes out: with loads and stores both in flight the counter
             cannot tell them apart, and each row's store would wait for the stores of the rows before it */
          asm volatile ("" : "+v" (km[j]));
        }
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j)
        { if (row + j >= rEnd) break;
          const U64 o = (row + j) * 64 + lane;
          const U64 bits = __ballot (f[j]);
          if (!DIRECT && lane == 0) { MgRankGrp g; g.bits = bits; g.rank = (U32) run; g.pad = 0; grp[row + j] = g; }
          if (f[j])
            { U64 idx = (U64) baseMax + 1 + run + (U32) __popcll (bits & below);
              if (idx < size)
                { __builtin_nontemporal_store (km[j], &value[idx]);
                  if (DIRECT) slots[slotId[o]].ord = (U32) idx | MG_ASSIGNED;
                }
            }
          run += (U32) __popcll (bits);
        }
    }
}

/* bit j of the result = bit 0 of byte j of q's 16 bytes (the multiplication gathers a word's four flag bits: no two of its partial products meet) */
__device__ __forceinline__ U32 mgFlagBits16 (const uint4 &q)
{
#define MG_NIB(w) ((((w) & 0x01010101u) * 0x00204081u >> 21) & 0xfu)
  return MG_NIB (q.x) | MG_NIB (q.y) << 4 | MG_NIB (q.z) << 8 | MG_NIB (q.w) << 12;
#undef MG_NIB
}

/* The bucketed leg's first half: the rank records alone, grp[row] = {the row's flags, the number of flags before the row} -- all that the
   rank lookups and the merge kernel need of the index assignment.  Same units as the count kernel; a lane takes a row, its 64 flag bytes in
   four 16-byte loads (flags is 16-byte aligned: mgTableAdd), so a wave does 64 rows a step with one scan and one store of 64 records. */
__global__ __launch_bounds__ (256)
void mgRankRecordKernel (const unsigned char *__restrict__ flags, U64 n, U64 rowsPerUnit, const U64 *__restrict__ unitBase, MgRankGrp *__restrict__ grp)
{
  MG_BUILD_PRIO ();
  const int lane = threadIdx.x & 63;
  const U64 unit = (U64) blockIdx.x * 4 + (U32) __builtin_amdgcn_readfirstlane ((int) (threadIdx.x >> 6));
  const U64 nRows = (n + 63) / 64;
  U64 row = unit * rowsPerUnit, rEnd = row + rowsPerUnit;
  if (rEnd > nRows) rEnd = nRows;
  if (row >= rEnd) return;
  U32 run = (U32) unitBase[unit];
  for ( ; row < rEnd ; row += 64)
    { const U64 r = row + lane;
      const bool in = r < rEnd;
      uint4 q[4] = {};
      if (in)
        { const uint4 *p = reinterpret_cast<const uint4 *> (flags + r * 64);
#pragma unroll
          for (int i = 0 ; i < 4 ; ++i) q[i] = p[i];
        }
      U64 bits = 0;
#pragma unroll
      for (int i = 0 ; i < 4 ; ++i) bits |= (U64) mgFlagBits16 (q[i]) << (16 * i);
      if (in && (r + 1) * 64 > n) bits &= ((U64) 1 << (n - r * 64)) - 1;      /* the last row of all: the bytes behind flags[n - 1] are nobody's */
      const U32 c = (U32) __popcll (bits), inc = mgWaveInclusiveSum (c);
      if (in) { MgRankGrp g; g.bits = bits; g.rank = run + inc - c; g.pad = 0; grp[r] = g; }
      run += (U32) __builtin_amdgcn_readlane ((int) inc, 63);
    }
}

/* The second half: value[baseMax + 1 + rank (o)] = kmer[o] for every flagged ordinal o, from the rank records -- a stream of k-mers in (dense,
   or SEG: still in the scan's segments) and values out that nothing later in the add reads, so it may run on a stream of its own beside the
   NEXT batch's scan (mgTableAdd).  For that it takes no LDS and few waves: the grid is whatever the launch says, the rows are cut into one
   contiguous piece per wave (rowsPerWave, a multiple of MG_RANK_ROWS), walked with MG_RANK_ROWS rows' loads in flight. */
template <bool SEG>
__global__ __launch_bounds__ (256)
void mgValueWriteKernel (const MgRankGrp *__restrict__ grp, const U64 *__restrict__ kmer, const MgSegSrc src, const MgSubSeg *__restrict__ subSeg,
                         U64 n, U64 rowsPerWave, U32 baseMax, U32 size, U64 *__restrict__ value)
{
  const int lane = threadIdx.x & 63;
  const U64 wave = (U64) blockIdx.x * 4 + (U32) __builtin_amdgcn_readfirstlane ((int) (threadIdx.x >> 6));
  const U64 nRows = (n + 63) / 64;
  U64 row = wave * rowsPerWave, rEnd = row + rowsPerWave;
  if (rEnd > nRows) rEnd = nRows;
  if (row >= rEnd) return;
  const U64 below = ((U64) 1 << lane) - 1;
  MgSegCursor cur; cur.w = 0; cur.s0 = 0; cur.s1 = 0;
  if (SEG) { mgSegCursorFrom (subSeg, row * 64 / MG_PART_SUB, &cur); mgSegCursorSeek (src, &cur, row * 64); }
  for ( ; row < rEnd ; row += MG_RANK_ROWS)
    { U64 km[MG_RANK_ROWS]; U64 bits[MG_RANK_ROWS]; U32 rank[MG_RANK_ROWS];
      /* all the record loads first (uniform), then all the k-mer loads, then the first use: with the segment walk's (uniform)
         branches between them the compiler otherwise waits for each row's loads -- and everything older -- in turn */
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j)
        { const MgRankGrp g = grp[row + j < rEnd ? row + j : row];
          bits[j] = g.bits; rank[j] = g.rank;
        }
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j)
        { const U64 o = (row + j) * 64 + lane;
          const bool in = (row + j < rEnd) && (o < n);
          if (SEG)
            { km[j] = 0;
              if (row + j < rEnd)                                            /* uniform (and then (row + j) * 64 < n) */
                { const U64 o0 = (row + j) * 64, last = o0 + 63 < n ? o0 + 63 : n - 1;
                  mgSegCursorSeek (src, &cur, o0);
                  const U64 *at = mgSegAddr (src, cur, o, last);
                  if (in) km[j] = __builtin_nontemporal_load (at);
                }
            }
          else km[j] = in ? __builtin_nontemporal_load (&kmer[o]) : 0;
        }
      /* every load has landed before the first store goes out: with loads and stores both in flight the counter
         cannot tell them apart, and each row's store would wait for the stores of the rows before it */
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j) asm volatile ("" : "+v" (km[j]));
#pragma unroll
      for (int j = 0 ; j < MG_RANK_ROWS ; ++j)
        { if (row + j >= rEnd) break;
          if ((bits[j] >> lane) & 1)                                         /* (a row's flags beyond n are 0) */
            { const U64 idx = (U64) baseMax + 1 + rank[j] + (U32) __popcll (bits[j] & below);
              if (idx < size) __builtin_nontemporal_store (km[j], &value[idx]);
            }
        }
    }
}

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

/* ======================================================================================== */
/* whole-table streaming passes (export / histogram)                                          */

/* pending depth counts -> delta16[idx-1], folded into baseDepth, cnt zeroed.  A workgroup takes whole buckets (R is no power of two:
   one occupancy test per bucket instead of a division per slot) */
__global__ void mgTableExportDepthKernel (MgSlot *__restrict__ slots, U32 nBuckets, const U32 *__restrict__ occ, U32 R,
                                          U16 *__restrict__ baseDepth, U16 *__restrict__ delta, U32 max)
{
  for (U32 bk = blockIdx.x ; bk < nBuckets ; bk += gridDim.x)
    { if (!occ[bk]) continue;
      MgSlot *base = slots + (U64) bk * R;
      for (U32 i = threadIdx.x ; i < R ; i += blockDim.x)
        { uint4 v = *reinterpret_cast<const uint4 *> (&base[i]);
          if (!(v.x | v.y) || !mgIsAssigned (v.z)) continue;
          U32 idx = v.z & ~MG_ASSIGNED, c = v.w;
          if (idx > max) continue;
          U32 cl = c > 0xffffu ? 0xffffu : c;
          delta[idx - 1] = (U16) cl;
          U32 b = (U32) baseDepth[idx] + cl;
          baseDepth[idx] = (U16) (b > 0xffffu ? 0xffffu : b);
          if (c) base[i].cnt = 0;
        }
    }
}

/* K5: histogram of min(65535, baseDepth + pending) over all entries (modutils.c:53-63) */
#define MG_HIST_LDS_BINS 8192
__global__ __launch_bounds__ (256)
void mgTableHistKernel (const MgSlot *__restrict__ slots, U32 nBuckets, const U32 *__restrict__ occ, U32 R,
                        const U16 *__restrict__ baseDepth, unsigned long long *__restrict__ hist)
{
  __shared__ U32 sBins[MG_HIST_LDS_BINS];
  for (int b = threadIdx.x ; b < MG_HIST_LDS_BINS ; b += blockDim.x) sBins[b] = 0;
  __syncthreads ();
  /* a workgroup takes whole buckets (one occupancy test per bucket) and keeps four 16-byte loads per lane in
     flight; whole waves run every step, so the two commonest bins (depth 1 and 2: sequencing errors) are counted
     per wave with ballots instead of 64 colliding LDS atomics */
  const int lane = threadIdx.x & 63;
  U32 n1 = 0, n2 = 0;
  for (U32 bk = blockIdx.x ; bk < nBuckets ; bk += gridDim.x)
    { if (!occ[bk]) continue;
      const MgSlot *base = slots + (U64) bk * R;
      for (U32 i0 = 0 ; i0 < R ; i0 += 4 * blockDim.x)
        { uint4 v[4];
#pragma unroll
          for (int j = 0 ; j < 4 ; ++j)
            { const U32 i = i0 + j * blockDim.x + threadIdx.x;
              v[j] = i < R ? *reinterpret_cast<const uint4 *> (&base[i]) : make_uint4 (0, 0, 0, 0);
            }
#pragma unroll
          for (int j = 0 ; j < 4 ; ++j)
            { U32 d = 0; bool have = false;
              if ((v[j].x | v[j].y) && mgIsAssigned (v[j].z))
                { U32 idx = v[j].z & ~MG_ASSIGNED;
                  d = (baseDepth ? (U32) baseDepth[idx] : 0u) + v[j].w;        /* baseDepth == 0: known to be all zero */
                  if (d > 0xffffu || d < v[j].w) d = 0xffffu;
                  have = true;
                }
              n1 += (U32) __popcll (__ballot (have && d == 1));
              n2 += (U32) __popcll (__ballot (have && d == 2));
              if (have && d != 1 && d != 2)
                { if (d < MG_HIST_LDS_BINS) atomicAdd (&sBins[d], 1u);
                  else atomicAdd (&hist[d], 1ull);
                }
            }
        }
    }
  if (lane == 0) { if (n1) atomicAdd (&sBins[1], n1); if (n2) atomicAdd (&sBins[2], n2); }
  __syncthreads ();
  for (int b = threadIdx.x ; b < MG_HIST_LDS_BINS ; b += blockDim.x)
    if (sBins[b]) atomicAdd (&hist[b], (unsigned long long) sBins[b]);
}

/* The reference's index[] layout (modset.c:45-62) rebuilt in parallel.  Sequential insertion in
 * index order puts entry i in the first slot of its probe sequence not held by an entry < i.
 * That layout is the unique one in which every slot an entry skipped holds a smaller index, so
 * it is reached by letting entries race with atomicMin: a smaller index evicts a larger one,
 * which then resumes its own probe sequence from where it sat.  Empty is 0xffffffff during the
 * race; mgIndexFinishKernel turns it into the reference's 0. */
__global__ void mgReplayIndexKernel (const U64 *__restrict__ value, U32 max, U64 factor1, int shift1,
                                     int tableBits, U32 *__restrict__ index)
{
  const U64 tmask = ((U64) 1 << tableBits) - 1;
  U64 i = 1 + (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; i <= max ; i += stride)
    { U32 cur = (U32) i;
      U64 hash = (value[cur] * factor1) >> shift1;
      U64 off = hash & tmask;
      U64 diff = ((hash >> tableBits) & tmask) | 1;
      for (;;)
        { U32 prev = atomicMin (&index[off], cur);
          if (prev == 0xffffffffu) break;
          if (prev > cur)
            { cur = prev;                               /* evicted entry continues from this slot */
              hash = (value[cur] * factor1) >> shift1;
              diff = ((hash >> tableBits) & tmask) | 1;
            }
          off = (off + diff) & tmask;
        }
    }
}

__global__ void mgIndexFinishKernel (U32 *__restrict__ index, U64 n)
{
  U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; i < n ; i += stride) if (index[i] == 0xffffffffu) index[i] = 0;
}

/* ======================================================================================== */
/* host side                                                                                  */

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
static void mgSetGeometry (MgTable *t, U64 want)
{
  U32 Rmax = t->wantR ? t->wantR : 4096;
  if (Rmax > 8192) Rmax = 8192;                   /* the dedup kernel's threads hold MG_DEDUP_PER (R <= 4096) or MG_DEDUP_PER_BIG slots each */
  if (Rmax < MG_R_QUANTUM) Rmax = MG_R_QUANTUM;
  if (want < MG_R_QUANTUM) want = MG_R_QUANTUM;
  int lgNB = 0;
  while (lgNB < 18 && (want + ((U64) 1 << lgNB) - 1) / ((U64) 1 << lgNB) > Rmax) ++lgNB;
  U64 R = (want + ((U64) 1 << lgNB) - 1) >> lgNB;
  R = (R + MG_R_QUANTUM - 1) / MG_R_QUANTUM * MG_R_QUANTUM;
  if (R > 8192) R = 8192;
  t->R = (U32) R; t->log2NB = lgNB; t->nSlots = R << lgNB;
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
  U32 Rown = t->wantR ? t->wantR : 4096;
  if (Rown > 8192) Rown = 8192;
  if (Rown < MG_R_QUANTUM) Rown = MG_R_QUANTUM;
  if (want < MG_R_QUANTUM) want = MG_R_QUANTUM;
  const U32 limits[2] = { Rown, 8192 };
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
    { if (attempt == 0 && exact) { t->log2NB = exactLg; t->R = exactR; t->nSlots = (U64) exactR << exactLg; }
      else if (attempt == 0) mgSetGeometry (t, want);
      else
        { int lg = 0; U32 R = 0;
          U32 *dFine = 0;
          if (hipMalloc ((void **) &dFine, sizeof (U32) << MG_FINE_LOG2) != hipSuccess) { s = mgHipFail (hipGetLastError (), "hipMalloc"); break; }
          if (hipMemsetAsync (dFine, 0, sizeof (U32) << MG_FINE_LOG2, st) != hipSuccess) { s = mgHipFail (hipGetLastError (), "hipMemsetAsync"); (void) hipFree (dFine); break; }
          const U32 oldNB = (U32) 1 << o.log2NB;
          MG_LAUNCH (MG_K_TABLE_HIST, st, mgFineCountSlotsKernel, dim3 (oldNB < 8192 ? oldNB : 8192), dim3 (256), 0, st, o.slots, oldNB, o.occ, o.R, t->kbits, keepMax, dFine);
          s = mgFitGeometry (t, dFine, want, &lg, &R, st);
          (void) hipFree (dFine);
          if (s) break;
          t->log2NB = lg; t->R = R; t->nSlots = (U64) R << lg;
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
/* the launchers: add, lookups, whole-table passes                                            */

#define MG_RANK_UNITS 8192           /* waves that share the ordered flag count */
static inline U64 mgRankRowsPerUnit (U64 n, U32 *nBlocks)
{
  U64 nRows = (n + 63) / 64;
  U64 per = (nRows + MG_RANK_UNITS - 1) / MG_RANK_UNITS; if (!per) per = 1;
  U64 units = (nRows + per - 1) / per; if (!units) units = 1;
  *nBlocks = (U32) ((units + 3) / 4);
  return per;
}

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

/* can mgTableAdd read this batch from the scan's segments?  Only the bucketed path does, and its first pass then
   needs the digit counts the scan made for exactly this table geometry */
bool mgTableAddTakesSegments (const MgTable *t, U64 n, const MgHistReq *counted)
{
  const int off = mgKnobs ()->noSegmentInput == 1;   /* test knob: always compact first */
  return !off && n && mgTableUseBuckets (t, n) && counted && counted->binCount && counted->log2NB == t->log2NB && counted->kbits == t->kbits && !counted->hiB;
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

/* The ordered count of flags[], for both legs of mgTableAdd: unitBase[] = the number of flags before every rank unit, counters[0] = the number of flags */
static MgStatus mgCountFlags (MgTable *t, const unsigned char *flags, U64 n, U64 *unitCount, U64 *unitBase, U32 *nBlocks, U64 *rows, hipStream_t st)
{
  *rows = mgRankRowsPerUnit (n, nBlocks);
  MG_LAUNCH (MG_K_RANK_COUNT, st, mgRankCountKernel, dim3 (*nBlocks), dim3 (256), 0, st, flags, n, *rows, unitCount);
  MG_LAUNCH (MG_K_RANK_SCAN, st, (mgGroupSumKernel<U64, U64>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, unitCount, unitBase, *nBlocks * 4, t->counters);
  return MG_OK;
}

/* The value writer of the bucketed leg (mgValueWriteKernel) on st: value[t->max + 1 + rank] = the k-mer of every flagged ordinal, from the rank records.
   waves: how many take the rows between them -- MG_VALUE_WAVES_ASIDE beside another kernel, MG_VALUE_WAVES_ALONE with the device to itself.
   segSrc != 0: the k-mers still sit in the scan's segments (subSeg: their cursors). */
#ifndef MG_VALUE_WAVES_ASIDE
#define MG_VALUE_WAVES_ASIDE 2048u   /* two waves a SIMD: what the next batch's scan leaves free */
#endif
#define MG_VALUE_WAVES_ALONE 8192u   /* as many as the rank units of the kernel this one was cut from */
static std::atomic<U64> gValueWriters[2];      /* launches since the process started: off the caller's stream, on it (mgValueWriterDiag) */
static MgStatus mgWriteValues (MgTable *t, const MgRankGrp *grp, const U64 *dKmer, const MgSegSrc *segSrc, const MgSubSeg *subSeg, U64 n, U32 waves, hipStream_t st)
{
  const MgSegSrc noSrc = {};
  const U64 nRows = (n + 63) / 64;
  U64 per = (nRows + waves - 1) / waves;
  per = (per + MG_RANK_ROWS - 1) / MG_RANK_ROWS * MG_RANK_ROWS;
  const U32 nBlocks = (U32) (((nRows + per - 1) / per + 3) / 4);
  if (segSrc) MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgValueWriteKernel<true>), dim3 (nBlocks), dim3 (256), 0, st, grp, (const U64 *) 0, *segSrc, subSeg, n, per, t->max, t->size, t->value);
  else MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgValueWriteKernel<false>), dim3 (nBlocks), dim3 (256), 0, st, grp, dKmer, noSrc, (const MgSubSeg *) 0, n, per, t->max, t->size, t->value);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}
extern "C" MgStatus mgValueWriterDiag (U64 *out2) { for (int i = 0 ; i < 2 ; ++i) out2[i] = gValueWriters[i].load (std::memory_order_relaxed); return MG_OK; }

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
  if (Rn < t->R) { t->R = (U32) Rn; t->nSlots = (U64) NB * Rn; }
  return MG_OK;
}

/* scratch needed by mgTableAdd for a batch of n */
size_t mgTableAddScratchBytes (const MgTable *t, U64 n)
{
  (void) t;
  U64 NB = (U64) 1 << 18;               /* the largest bucket count: the table may grow between passes of one call */
  size_t rank = mgAl256 (n) /*flags*/ + 2 * mgAl256 ((MG_RANK_UNITS + 8) * 8) + mgAl256 ((n / 64 + 2) * sizeof (MgRankGrp));
  size_t direct = mgAl256 (n * 4);
  size_t part = 2 * (mgAl256 (n * 8) + mgAl256 (n * 4)) + mgAl256 (n * 4)
              + mgAl256 ((NB + 2) * 8) * 3 + mgAl256 ((NB + 2) * 4) * 2 + mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8) * 3 + 2 * mgAl256 ((U64) MG_PART_MAXBINS * 16 * 8 + 4096)
              + mgAl256 ((MG_PART_MAXBINS + 2) * 4) + mgAl256 ((MG_PART_MAXBINS + 2 + n / MG_PART_CHUNK + MG_PART_MAXBINS + 2) * 4)
              + mgAl256 ((size_t) (MG_RANK_GROUPS + 2) * NB * sizeof (unsigned short)) + mgAl256 ((n / MG_PART_SUB + 2) * 24)
              + mgAl256 (mgHotItemsCap (n) * 8) + mgAl256 (mgHotItemsCap (n) * 4) + 256;
  return rank + (direct > part ? direct : part) + 4096;
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
  char *wb = (char *) scratch;
  unsigned char *flags = (unsigned char *) wb;       wb += mgAl256 (n);
  U64 *blockCount = (U64 *) wb;                      wb += mgAl256 ((MG_RANK_UNITS + 8) * 8);
  U64 *blockBase = (U64 *) wb;                       wb += mgAl256 ((MG_RANK_UNITS + 8) * 8);
  MgRankGrp *grp = (MgRankGrp *) wb;                 wb += mgAl256 ((n / 64 + 2) * sizeof (MgRankGrp));
  MG_HIP (hipMemsetAsync (blockCount, 0, (MG_RANK_UNITS + 8) * 8, st));

  if (!mgTableUseBuckets (t, n))
    { U32 *slotId = (U32 *) wb;
      if (aside) { mgSetError ("internal: the direct insert has no value writer to run aside"); return MG_ERR_ARG; }      /* (it writes value[] on st: the caller decides by mgTableUseBuckets too, and orders st itself) */
      { MgStatus cs = mgTableClean (t, st); if (cs) return cs; }
      MG_LAUNCH (MG_K_TABLE_INSERT, st, mgTableInsertKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, t->slots, g, dKmer, n, slotId, withDepth, t->counters);
      MG_LAUNCH (MG_K_TABLE_FLAG, st, mgDirectFlagKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, t->slots, slotId, n, flags);
      { U32 nBlocks; U64 rows;
        MgStatus as = mgCountFlags (t, flags, n, blockCount, blockBase, &nBlocks, &rows, st); if (as) return as;
        MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgRankAssignKernel<true>), dim3 (nBlocks), dim3 (256), 0, st,
                   flags, dKmer, n, rows, blockBase, t->max, t->size, t->value, t->slots, slotId, grp);
      }
      MG_HIP (hipGetLastError ());
      /* occ[] is kept exact only by the bucketed path and the loader; the direct path marks buckets non-empty */
      return mgTableMarkOccupied (t, dKmer, n, st);
    }

  /* ---- bucketed ---- */
  const U64 NB = (U64) 1 << t->log2NB;
  U64 *kA = (U64 *) wb;  wb += mgAl256 (n * 8);
  U32 *tA = (U32 *) wb;  wb += mgAl256 (n * 4);
  U64 *kB = (U64 *) wb;  wb += mgAl256 (n * 8);
  U32 *tB = (U32 *) wb;  wb += mgAl256 (n * 4);
  U32 *cB = (U32 *) wb;  wb += mgAl256 (n * 4);
  U64 *fineStart = (U64 *) wb;                wb += mgAl256 ((NB + 2) * 8);
  unsigned long long *fineCursor = (unsigned long long *) wb; wb += mgAl256 ((NB + 2 + (U64) MG_PART_MAXBINS * 16) * 8);
  /* spare64 */                               wb += mgAl256 ((NB + 2) * 8);      /* unused: its bytes stay in the layout */
  U32 *fineCount = (U32 *) wb;                wb += mgAl256 ((NB + 2) * 4);
  U32 *uniqCount = (U32 *) wb;                wb += mgAl256 ((NB + 2) * 4);
  U64 *coarseStart = (U64 *) wb;              wb += mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8);
  unsigned long long *coarseCursor = (unsigned long long *) wb; wb += mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8 * 16);
  U64 *whole = (U64 *) wb;                    wb += mgAl256 (((U64) MG_PART_MAXBINS + 2) * 8);
  U32 *coarseCount = (U32 *) wb;              wb += mgAl256 ((MG_PART_MAXBINS + 2) * 4);
  U32 *chunkBase = (U32 *) wb;                wb += mgAl256 ((MG_PART_MAXBINS + 2 + n / MG_PART_CHUNK + MG_PART_MAXBINS + 2) * 4);   /* + the segment of every chunk */
  unsigned short *sliceOff = (unsigned short *) wb;   wb += mgAl256 ((size_t) (MG_RANK_GROUPS + 2) * NB * sizeof (unsigned short));
  MgSubSeg *subSeg = (MgSubSeg *) wb;         wb += mgAl256 ((n / MG_PART_SUB + 2) * sizeof (MgSubSeg));
  U64 *hotItems = (U64 *) wb;                 wb += mgAl256 (mgHotItemsCap (n) * 8);
  U32 *hotBuckets = (U32 *) wb;               wb += mgAl256 (mgHotItemsCap (n) * 4);
  unsigned long long *hotCount = (unsigned long long *) wb; wb += 256;

  MgAddPlan plan;
  mgAddPlan (t, n, wasEmpty, &plan);
  const int hiB = plan.hiB, loB = plan.loB;
  const U32 *pre = (counted && counted->binCount && counted->log2NB == t->log2NB && counted->kbits == t->kbits && !counted->hiB) ? counted->binCount : 0;
  U64 segInit[2] = { 0, n };
  MG_HIP (hipMemcpyAsync (whole, segInit, 16, hipMemcpyHostToDevice, st));
  MgStatus s;
  MgPartPassArgs p1 = {};                /* the first pass: the batch, dense or in the scan's segments, by the coarse digit -- the only digit of a table of few buckets */
  p1.inMode = segSrc ? MG_EL_SEG : MG_EL_DENSE; p1.packed = plan.packed; p1.f = plan.f; p1.kIn = dKmer; p1.n = n; p1.segStart = whole; p1.nSeg = 1;
  p1.nBins = (U32) 1 << hiB; p1.chunkBase = chunkBase; p1.counted = pre; p1.segSrc = segSrc; p1.subSeg = subSeg;
  if (!loB)
    { p1.kOut = kB; p1.tOut = tB; p1.binStart = fineStart; p1.cursor = fineCursor; p1.binCount = fineCount;
      if ((s = mgPartPass (t, p1, st))) return s;
    }
  else
    { /* the first pass leaves every element's fine digit in a byte beside it (in cB, which the dedup kernel only writes later) */
      unsigned char *digits = plan.digitBytes ? reinterpret_cast<unsigned char *> (cB) : 0;
      p1.shift = loB; p1.kOut = kA; p1.tOut = tA; p1.binStart = coarseStart; p1.cursor = coarseCursor; p1.binCount = coarseCount;
      p1.digitOut = digits; p1.nextBins = (U32) 1 << loB;
      if ((s = mgPartPass (t, p1, st))) return s;
      MgPartPassArgs p2 = {};            /* the second pass: every coarse bin by the fine digit, into the buckets */
      p2.inMode = plan.packed ? MG_EL_PACKED : MG_EL_WIDE; p2.packed = plan.packed; p2.f = plan.f; p2.kIn = kA; p2.tIn = tA; p2.n = n; p2.segStart = coarseStart; p2.nSeg = (U32) 1 << hiB;
      p2.nBins = (U32) 1 << loB; p2.kOut = kB; p2.tOut = tB; p2.binStart = fineStart; p2.cursor = fineCursor; p2.binCount = fineCount; p2.chunkBase = chunkBase;
      p2.digitIn = digits;
      if ((s = mgPartPass (t, p2, st))) return s;
    }

  MG_HIP (hipMemsetAsync (flags, plan.markDup ? 1 : 0, n, st));
  MgBucketArgs a;
  a.slots = t->slots; a.g = g; a.nBuckets = (U32) NB; a.bucketStart = fineStart;
  a.pK = kB; a.pT = tB; a.pC = cB; a.uniqCount = uniqCount; a.occ = t->occ; a.flags = flags;
  a.grp = grp; a.baseMax = t->max; a.size = t->size; a.withDepth = withDepth;
  a.markDup = plan.markDup; a.slotShift = plan.slotShift; a.place = plan.place;
  a.sliceShift = plan.sliceShift; a.nSlices = plan.nSlices; a.sliceOff = sliceOff;
  a.hotSplit = plan.hotSplit; a.hotChunk = plan.hotChunk; a.hotItems = hotItems; a.hotCount = hotCount; a.hotBuckets = hotBuckets;
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
    { if ((s = mgAddTighten (t, plan.tightPct, uniqCount, &fullest, st))) return s;
      if (t->R != a.g.R) { a.g = mgGeomOf (t); lds = mgMergeLdsBytes (t->R); }
    }
  /* index assignment in two halves.  The rank records are all the rest of the add needs; value[] is read by nobody before the caller looks at the
     set, so with `aside` its writer -- a plain stream over 2 GB -- goes behind the merge kernel onto a stream of its own, where it runs beside
     whatever the caller starts next: the scan of the next batch, which leaves the memory path idle.  (Beside the lookups or the merge of this add
     it cost more than it hid: they want the memory path themselves.) */
  { U32 nBlocks; U64 rows;
    if ((s = mgCountFlags (t, flags, n, blockCount, blockBase, &nBlocks, &rows, st))) return s;
    MG_LAUNCH (MG_K_RANK_RECORD, st, mgRankRecordKernel, dim3 (nBlocks), dim3 (256), 0, st, flags, n, rows, blockBase, grp);
  }
  if (!aside && (s = mgWriteValues (t, grp, dKmer, segSrc, subSeg, n, MG_VALUE_WAVES_ALONE, st))) return s;
  if ((s = mgRankLookup (a, st))) return s;
  if ((s = mgBucketMerge (a, fullest, bThreads, bGrid, perBlock, lds, st))) return s;
  MG_HIP (hipGetLastError ());
  if (aside)
    { MG_HIP (hipEventRecord (aside->merged, st));
      MG_HIP (hipStreamWaitEvent (aside->stream, aside->merged, 0));
      if ((s = mgWriteValues (t, grp, dKmer, segSrc, subSeg, n, MG_VALUE_WAVES_ASIDE, aside->stream))) return s;
      MG_HIP (hipEventRecord (aside->done, aside->stream));
      aside->launched = true;
    }
  gValueWriters[aside ? 0 : 1].fetch_add (1, std::memory_order_relaxed);
  return MG_OK;
}

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
  U32 *dFine = 0;
  if (hipMalloc ((void **) &dFine, sizeof (U32) << MG_FINE_LOG2) != hipSuccess) return mgHipFail (hipGetLastError (), "hipMalloc");
  if (hipMemsetAsync (dFine, 0, sizeof (U32) << MG_FINE_LOG2, st) != hipSuccess) s = mgHipFail (hipGetLastError (), "hipMemsetAsync");
  else
    { MG_LAUNCH (MG_K_TABLE_HIST, st, mgFineCountValuesKernel, dim3 (mgGridWide (last)), dim3 (256), 0, st, dValue, 1u, last, t->kbits, dFine);
      s = mgFitGeometry (t, dFine, mgSlotsFor (t, last), &lg, &R, st);
    }
  (void) hipFree (dFine);
  if (!s) s = mgTableRehashExact (t, lg, R, st);
  if (s) return s;
  if ((s = mgLoadLaunch (t, dValue, first, last, st, &over))) return s;
  if (over) { mgSetError ("internal: the device table's fitted geometry (2^%d x %u) does not hold the host's entries", lg, R); return MG_ERR_CAPACITY; }
  return MG_OK;
}

MgStatus mgTableExportDepth (MgTable *t, U16 *dDelta, hipStream_t st)
{
  if (!t->max) return MG_OK;
  MG_HIP (hipMemsetAsync (dDelta, 0, (size_t) t->max * sizeof (U16), st));
  t->baseZero = false;                                   /* the fold below writes baseDepth */
  t->pendingDepth = false;
  t->liveHistValid = false;
  { const U32 NB = (U32) 1 << t->log2NB;
    MG_LAUNCH (MG_K_TABLE_EXPORT, st, mgTableExportDepthKernel, dim3 (NB < 8192 ? NB : 8192), dim3 (256), 0, st,
               t->slots, NB, t->occ, t->R, t->baseDepth, dDelta, t->max);
  }
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

/* dHist[i] += live[i] */
__global__ void mgHistAddKernel (const U64 *__restrict__ live, unsigned long long *__restrict__ hist)
{ U32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i < 65536 && live[i]) atomicAdd (&hist[i], (unsigned long long) live[i]); }

MgStatus mgTableHistogram (MgTable *t, U64 *dHist, hipStream_t st)
{
  if (!t->max) return MG_OK;
  if (t->liveHistValid && t->liveHist)                 /* the merge kernel kept it while it built the set */
    { MG_LAUNCH (MG_K_TABLE_HIST, st, mgHistAddKernel, dim3 (256), dim3 (256), 0, st, t->liveHist, (unsigned long long *) dHist);
      MG_HIP (hipGetLastError ());
      return MG_OK;
    }
  { const U32 NB = (U32) 1 << t->log2NB;
    MG_LAUNCH (MG_K_TABLE_HIST, st, mgTableHistKernel, dim3 (NB < 2048 ? NB : 2048), dim3 (256), 0, st,
               t->slots, NB, t->occ, t->R, t->baseZero ? (const U16 *) 0 : t->baseDepth, (unsigned long long *) dHist);
  }
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

MgStatus mgTableReplayIndex (MgTable *t, const MgHashParams &p, int tableBits, U32 *dIndex, hipStream_t st)
{
  U64 n = (U64) 1 << tableBits;
  MG_HIP (hipMemsetAsync (dIndex, 0xff, n * sizeof (U32), st));
  if (t->max)
    { MG_LAUNCH (MG_K_INDEX_REPLAY, st, mgReplayIndexKernel, dim3 (mgGridWide (t->max)), dim3 (256), 0, st,
                          t->value, t->max, p.factor1, p.shift1, tableBits, dIndex);
      MG_HIP (hipGetLastError ());
    }
  MG_LAUNCH (MG_K_INDEX_FINISH, st, mgIndexFinishKernel, dim3 (mgGrid (n, 256, 8192)), dim3 (256), 0, st, dIndex, n);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

/* ======================================================================================== */
/* whole-set passes on the device: merge (modset.c:106-128) and depth prune (modset.c:64-77)  */

/* after ms2's values were inserted (idx[i] = their index in ms1): depth adds saturate at 65535;
 * copy bits add and saturate at 3 while the entry's other info bits are cleared (modset.c:120-126) */
__global__ void mgMergeApplyKernel (const U32 *__restrict__ idx, const U16 *__restrict__ depth2, const U8 *__restrict__ info2,
                                    U32 n2, U16 *__restrict__ baseDepth, U8 *__restrict__ info1)
{
  U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; i < n2 ; i += stride)
    { U32 j = idx[i];
      if (!j) continue;
      U32 d = (U32) baseDepth[j] + depth2[i];
      baseDepth[j] = (U16) (d > 0xffffu ? 0xffffu : d);
      U32 a = info1[j] & 3, c = a + (info2[i] & 3);
      if (c > 3) c = 3;
      info1[j] = (U8) (a | c);
    }
}

/* keep[i-1] = 1 when entry i survives the prune */
__global__ void mgPruneFlagKernel (const U16 *__restrict__ depth, U32 n, int lo, int hi, unsigned char *__restrict__ keep)
{
  U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; i < n ; i += stride)
    { int d = depth[i + 1];
      keep[i] = (d >= lo && (!hi || d < hi)) ? 1 : 0;
    }
}

/* depth/info of the survivors move to their new index (rank structure from mgRankAssignKernel<false>) */
__global__ void mgPruneMoveKernel (const unsigned char *__restrict__ keep, const MgRankGrp *__restrict__ grp, U32 n,
                                   const U16 *__restrict__ depth, const U8 *__restrict__ info,
                                   U16 *__restrict__ newDepth, U8 *__restrict__ newInfo)
{
  U64 i = (U64) blockIdx.x * blockDim.x + threadIdx.x;
  const U64 stride = (U64) gridDim.x * blockDim.x;
  for ( ; i < n ; i += stride)
    { if (!keep[i]) continue;
      MgRankGrp g = grp[i >> 6];
      U32 r = 1 + g.rank + (U32) __popcll (g.bits & (((U64) 1 << (i & 63)) - 1));
      newDepth[r] = depth[i + 1]; newInfo[r] = info[i + 1];
    }
}

MgStatus mgTableMergeApply (const U32 *dIdx, const U16 *dDepth2, const U8 *dInfo2, U32 n2, U16 *dBaseDepth, U8 *dInfo1, hipStream_t st)
{
  if (!n2) return MG_OK;
  MG_LAUNCH (MG_K_TABLE_EXPORT, st, mgMergeApplyKernel, dim3 (mgGridWide (n2)), dim3 (256), 0, st, dIdx, dDepth2, dInfo2, n2, dBaseDepth, dInfo1);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}

size_t mgTablePruneScratchBytes (U32 n)
{ return mgAl256 (n) + 2 * mgAl256 ((MG_RANK_UNITS + 8) * 8) + mgAl256 (((U64) n / 64 + 2) * sizeof (MgRankGrp)) + 4096; }

/* survivors of (lo <= depth < hi) keep their relative order: newValue/newDepth/newInfo[1..*]; counters[0] = how many */
MgStatus mgTablePrune (MgTable *t, const U8 *dInfo, int lo, int hi, U64 *dNewValue, U16 *dNewDepth, U8 *dNewInfo,
                       void *scratch, hipStream_t st)
{
  const U32 n = t->max;
  MG_HIP (hipMemsetAsync (t->counters, 0, 16, st));
  if (!n) return MG_OK;
  char *wb = (char *) scratch;
  unsigned char *keep = (unsigned char *) wb;        wb += mgAl256 (n);
  U64 *unitCount = (U64 *) wb;                       wb += mgAl256 ((MG_RANK_UNITS + 8) * 8);
  U64 *unitBase = (U64 *) wb;                        wb += mgAl256 ((MG_RANK_UNITS + 8) * 8);
  MgRankGrp *grp = (MgRankGrp *) wb;
  U32 nBlocks; U64 rows = mgRankRowsPerUnit (n, &nBlocks);
  MG_HIP (hipMemsetAsync (unitCount, 0, (MG_RANK_UNITS + 8) * 8, st));
  MG_LAUNCH (MG_K_TABLE_FLAG, st, mgPruneFlagKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, t->baseDepth, n, lo, hi, keep);
  MG_LAUNCH (MG_K_RANK_COUNT, st, mgRankCountKernel, dim3 (nBlocks), dim3 (256), 0, st, keep, (U64) n, rows, unitCount);
  MG_LAUNCH (MG_K_RANK_SCAN, st, (mgGroupSumKernel<U64, U64>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, unitCount, unitBase, nBlocks * 4, t->counters);
  /* value[i+1] of survivor i -> newValue[1 + rank]: the assign kernel with "kmer" = value + 1, base 0 */
  MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgRankAssignKernel<false>), dim3 (nBlocks), dim3 (256), 0, st,
             keep, t->value + 1, (U64) n, rows, unitBase, 0u, 0xffffffffu, dNewValue, t->slots, (const U32 *) 0, grp);
  MG_LAUNCH (MG_K_TABLE_EXPORT, st, mgPruneMoveKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, keep, grp, n, t->baseDepth, dInfo, dNewDepth, dNewInfo);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}
