/* mg_tableset.hip — the passes over a whole set in the device modset table (mg_table.hip: the layout): the pending depths exported
 * (mgTableExportDepth), the depth histogram (mgTableHistogram), the reference's index[] replayed (mgTableReplayIndex), and the two that
 * make a set from sets: what a merge adds to the entries it met (mgTableMergeApply) and the depth prune (mgTablePrune), whose survivors
 * are numbered by the ordered flag count of mg_rank.hip. */
#include "mg_table.h"

/* ======================================================================================== */
/* whole-table streaming passes (export / histogram / index replay)                           */

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

size_t mgTablePruneScratchBytes (U32 n) { return mgRankCarve (0, n, 0) + 4096; }

/* survivors of (lo <= depth < hi) keep their relative order: newValue/newDepth/newInfo[1..*]; counters[0] = how many */
MgStatus mgTablePrune (MgTable *t, const U8 *dInfo, int lo, int hi, U64 *dNewValue, U16 *dNewDepth, U8 *dNewInfo,
                       void *scratch, hipStream_t st)
{
  const U32 n = t->max;
  MG_HIP (hipMemsetAsync (t->counters, 0, 16, st));
  if (!n) return MG_OK;
  MgRankBufs keep;                                   /* keep.flags[i] = 1: entry i + 1 survives */
  MgStatus s;
  (void) mgRankCarve (scratch, n, &keep);
  MG_LAUNCH (MG_K_TABLE_FLAG, st, mgPruneFlagKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, t->baseDepth, n, lo, hi, keep.flags);
  if ((s = mgRankCount (t, keep, n, st)) || (s = mgRankAssignPrune (t, keep, n, dNewValue, st))) return s;
  MG_LAUNCH (MG_K_TABLE_EXPORT, st, mgPruneMoveKernel, dim3 (mgGridWide (n)), dim3 (256), 0, st, keep.flags, keep.grp, n, t->baseDepth, dInfo, dNewDepth, dNewInfo);
  MG_HIP (hipGetLastError ());
  return MG_OK;
}
