/* mg_rank.hip — the ordered flag count of the device modset table: flags[o] = 1 marks the ordinals that get an index (both legs of
 * mgTableAdd: the first occurrence of every new k-mer) or that stay (mgTablePrune: the survivors), and flagged ordinal o gets
 * base + 1 + the number of flags before o.
 *
 * The ordinal range is cut into contiguous pieces, one per wave ("rank unit"); a wave walks its piece in rows of 64 ordinals, so
 * flags, k-mers and the value[] it writes are all lane-contiguous.  Pass A counts per unit (mgRankCount), a one-block scan turns the
 * counts into bases, pass B assigns: in one kernel (mgRankAssignDirect, mgRankAssignPrune), or in two halves, the rank records
 * (mgRankRecord) and the values written from them (mgWriteValues).
 *
 * The host entry points at the end of the file are the only way in (declared in mg_table.h); what the passes share -- the four buffers
 * (MgRankBufs, mgRankCarve), the units and the rows of a unit -- is decided here and nowhere else. */
#include <atomic>
#include "mg_table.h"

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

/* ======================================================================================== */
/* host side: the only way in                                                                 */

#define MG_RANK_UNITS 8192           /* waves that share the ordered flag count */
static inline U64 mgRankRowsPerUnit (U64 n, U32 *nBlocks)
{
  U64 nRows = (n + 63) / 64;
  U64 per = (nRows + MG_RANK_UNITS - 1) / MG_RANK_UNITS; if (!per) per = 1;
  U64 units = (nRows + per - 1) / per; if (!units) units = 1;
  *nBlocks = (U32) ((units + 3) / 4);
  return per;
}

/* the four buffers of a count over n flags, carved from base on (256-byte aligned: mgRankRecordKernel reads flags[] 16 bytes at a time);
   returns their bytes.  base 0: only measures (r may be 0 too) */
size_t mgRankCarve (void *base, U64 n, MgRankBufs *r)
{
  MgRankBufs b; size_t at = 0;
  b.flags = mgCarve<unsigned char> (base, &at, n);
  b.unitCount = mgCarve<U64> (base, &at, MG_RANK_UNITS + 8);
  b.unitBase = mgCarve<U64> (base, &at, MG_RANK_UNITS + 8);
  b.grp = mgCarve<MgRankGrp> (base, &at, n / 64 + 2);
  if (r) *r = b;
  return at;
}

/* pass A and the scan: unitBase[] = the number of flags before every rank unit, counters[0] = the number of flags.  unitCount[] needs no
   preset: the count kernel's grid is nBlocks workgroups of four waves, every wave stores its unit's count whether or not the unit has
   rows, and mgGroupSumKernel reads exactly those nBlocks * 4 words -- as the kernels of pass B read unitBase[] of no other unit */
MgStatus mgRankCount (MgTable *t, const MgRankBufs &r, U64 n, hipStream_t st)
{
  U32 nBlocks; const U64 rows = mgRankRowsPerUnit (n, &nBlocks);
  MG_LAUNCH (MG_K_RANK_COUNT, st, mgRankCountKernel, dim3 (nBlocks), dim3 (256), 0, st, r.flags, n, rows, r.unitCount);
  MG_LAUNCH (MG_K_RANK_SCAN, st, (mgGroupSumKernel<U64, U64>), dim3 (1), dim3 (MG_GROUP_THREADS), 0, st, r.unitCount, r.unitBase, nBlocks * 4, t->counters);
  return MG_OK;
}

/* pass B of the bucketed leg, first half: r.grp[] from r.flags and r.unitBase */
MgStatus mgRankRecord (const MgRankBufs &r, U64 n, hipStream_t st)
{
  U32 nBlocks; const U64 rows = mgRankRowsPerUnit (n, &nBlocks);
  MG_LAUNCH (MG_K_RANK_RECORD, st, mgRankRecordKernel, dim3 (nBlocks), dim3 (256), 0, st, r.flags, n, rows, r.unitBase, r.grp);
  return MG_OK;
}

/* pass B of the direct leg: value[t->max + 1 + rank] = dKmer[o] and the index into slot slotId[o], for every flagged ordinal o */
MgStatus mgRankAssignDirect (MgTable *t, const MgRankBufs &r, const U64 *dKmer, const U32 *slotId, U64 n, hipStream_t st)
{
  U32 nBlocks; const U64 rows = mgRankRowsPerUnit (n, &nBlocks);
  MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgRankAssignKernel<true>), dim3 (nBlocks), dim3 (256), 0, st,
             r.flags, dKmer, n, rows, r.unitBase, t->max, t->size, t->value, t->slots, slotId, r.grp);
  return MG_OK;
}

/* pass B of mgTablePrune: value[i + 1] of survivor i -> dNewValue[1 + rank] (the assign kernel with "kmer" = value + 1, base 0), and the
   rank records in r.grp[] for the pass that moves the depths */
MgStatus mgRankAssignPrune (MgTable *t, const MgRankBufs &r, U64 n, U64 *dNewValue, hipStream_t st)
{
  U32 nBlocks; const U64 rows = mgRankRowsPerUnit (n, &nBlocks);
  MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgRankAssignKernel<false>), dim3 (nBlocks), dim3 (256), 0, st,
             r.flags, t->value + 1, n, rows, r.unitBase, 0u, 0xffffffffu, dNewValue, t->slots, (const U32 *) 0, r.grp);
  return MG_OK;
}

/* The value writer of the bucketed leg (mgValueWriteKernel) on st: value[t->max + 1 + rank] = the k-mer of every flagged ordinal, from the rank records.
   aside: st is a stream of the writer's own and another kernel runs beside it -- MG_VALUE_WAVES_ASIDE waves take the rows between them; otherwise
   it has the device to itself, MG_VALUE_WAVES_ALONE.  segSrc != 0: the k-mers still sit in the scan's segments (subSeg: their cursors). */
#ifndef MG_VALUE_WAVES_ASIDE
#define MG_VALUE_WAVES_ASIDE 2048u   /* two waves a SIMD: what the next batch's scan leaves free */
#endif
#define MG_VALUE_WAVES_ALONE 8192u   /* as many as the rank units of the kernel this one was cut from */
static std::atomic<U64> gValueWriters[2];      /* launches since the process started: off the caller's stream, on it (mgValueWriterDiag) */
MgStatus mgWriteValues (MgTable *t, const MgRankGrp *grp, const U64 *dKmer, const MgSegSrc *segSrc, const MgSubSeg *subSeg, U64 n, bool aside, hipStream_t st)
{
  const MgSegSrc noSrc = {};
  const U32 waves = aside ? MG_VALUE_WAVES_ASIDE : MG_VALUE_WAVES_ALONE;
  const U64 nRows = (n + 63) / 64;
  U64 per = (nRows + waves - 1) / waves;
  per = (per + MG_RANK_ROWS - 1) / MG_RANK_ROWS * MG_RANK_ROWS;
  const U32 nBlocks = (U32) (((nRows + per - 1) / per + 3) / 4);
  if (segSrc) MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgValueWriteKernel<true>), dim3 (nBlocks), dim3 (256), 0, st, grp, (const U64 *) 0, *segSrc, subSeg, n, per, t->max, t->size, t->value);
  else MG_LAUNCH (MG_K_TABLE_ASSIGN, st, (mgValueWriteKernel<false>), dim3 (nBlocks), dim3 (256), 0, st, grp, dKmer, noSrc, (const MgSubSeg *) 0, n, per, t->max, t->size, t->value);
  MG_HIP (hipGetLastError ());
  gValueWriters[aside ? 0 : 1].fetch_add (1, std::memory_order_relaxed);
  return MG_OK;
}
extern "C" MgStatus mgValueWriterDiag (U64 *out2) { for (int i = 0 ; i < 2 ; ++i) out2[i] = gValueWriters[i].load (std::memory_order_relaxed); return MG_OK; }
