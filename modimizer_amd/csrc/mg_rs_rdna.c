/* mg_rs_rdna.c — modasm -R / -T / -rb over a read set: refFlag (modasm.c:752-860), testMods (595-748), resetBits (864-908).
 * ModInfo, the reads' otherFlags and the reference's static RUN are kept beside the set, keyed by its address (MgReadset's layout is pinned), and go with
 * mgReadsetDestroy.  Every pass works on copies of info[] and ModInfo and commits them when nothing can fail any more: on -1 nothing is modified. */
#include <pthread.h>
#include "mg_readset_int.h"

typedef struct RdnaState { const MgReadset *rs; MgModInfo *mi; size_t nMi; U8 *flags; int capFlags, run; struct RdnaState *next; } RdnaState;
static pthread_mutex_t gRdnaLock = PTHREAD_MUTEX_INITIALIZER;
static RdnaState *gRdna;
static __thread int gRdnaPath = -1;
static __thread U64 gRdnaDiag[4];
static __thread U32 gRdnaGrid[4];
int mgReadsetRdnaPath (void) { return gRdnaPath; }
void mgReadsetRdnaDiag (U64 out4[4]) { memcpy (out4, gRdnaDiag, sizeof (gRdnaDiag)); }
void mgReadsetRdnaGrid (U32 out4[4]) { memcpy (out4, gRdnaGrid, sizeof (gRdnaGrid)); }

static RdnaState *rdnaState (const MgReadset *rs, int create)
{
  pthread_mutex_lock (&gRdnaLock);
  RdnaState *s = gRdna;
  while (s && s->rs != rs) s = s->next;
  if (!s && create) { s = (RdnaState *) calloc (1, sizeof (RdnaState)); s->rs = rs; s->next = gRdna; gRdna = s; }
  pthread_mutex_unlock (&gRdnaLock);
  return s;
}
void mgRsRdnaForget (const MgReadset *rs)
{
  pthread_mutex_lock (&gRdnaLock);
  for (RdnaState **p = &gRdna ; *p ; p = &(*p)->next)
    if ((*p)->rs == rs) { RdnaState *s = *p; *p = s->next; free (s->mi); free (s->flags); free (s); break; }
  pthread_mutex_unlock (&gRdnaLock);
}
/* otherFlags[0 .. nReads], zero for the reads that came since it was last asked for */
static U8 *rdnaFlags (RdnaState *s, const MgReadset *rs)
{
  if (s->capFlags < rs->nReads + 1)
    { s->flags = (U8 *) realloc (s->flags, (size_t) rs->nReads + 1);
      memset (s->flags + s->capFlags, 0, (size_t) (rs->nReads + 1 - s->capFlags));
      s->capFlags = rs->nReads + 1;
    }
  return s->flags;
}
const MgModInfo *mgReadsetModInfo (const MgReadset *rs) { RdnaState *s = rdnaState (rs, 0); return s ? s->mi : 0; }
U8 *mgRsRdnaFlagsOf (const MgReadset *rs, int create) { RdnaState *s = rdnaState (rs, create); return s ? rdnaFlags (s, rs) : 0; }
const U8 *mgReadsetReadFlags (const MgReadset *rs) { return mgRsRdnaFlagsOf (rs, 1); }
int mgReadsetTestModsRun (const MgReadset *rs) { RdnaState *s = rdnaState (rs, 0); return s ? s->run : 0; }

#define MG_RDNA_DEVICE_MIN ((U64) 1 << 21)
enum { RD_REF = 1, RD_CORE = 2, RD_VAR = 4, RD_MULTI = 8 };        /* modasm.c:61-70 */
static U8 rdnaDepthClass (int depth) { return depth > 4750 ? RD_MULTI : depth > 2750 ? RD_CORE : RD_VAR; }      /* modasm.c:770-772,821-823 */

static void rdnaN200Host (const MgReadset *rs, const U8 *qual, int *n200, int *m200)      /* modasm.c:781-802 */
{
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { const U32 *hit = rs->hit + rs->hitStart[i];
      const int nHit = (int) (rs->hitStart[i + 1] - rs->hitStart[i]);
      int n = 0; n200[i] = m200[i] = 0;
      for (int j = 0 ; j < nHit ; ++j) if (qual[hit[j] & TOPMASK] && ++n == 200) { n200[i] = j; break; }
      if (!n200[i]) continue;
      n = 0;
      for (int j = nHit ; --j ; ) if (qual[hit[j] & TOPMASK] && ++n == 200) { m200[i] = j; break; }
    }
}

int mgReadsetRefFlagHits (MgReadset *rs, const U32 *index, const int *pos, U64 n, FILE *out)
{
  gRdnaPath = -1;
  Modset *ms = rs->ms;
  if (modsetSyncToHost (ms, 0)) return -1;
  const size_t m = (size_t) ms->max + 1;
  for (U64 j = 0 ; j < n ; ++j)
    if (!index[j] || index[j] > ms->max) { char msg[160]; snprintf (msg, sizeof (msg), "-R: hit %llu names mod %u, the set holds 1 .. %u", (unsigned long long) j, index[j], ms->max); mgSetErrorText (msg); return -1; }
  RdnaState *s = rdnaState (rs, 1);
  if (s->mi && s->nMi != m) { mgSetErrorText ("-R: the modset has changed its size since the first -R"); return -1; }
  MgModInfo *mi = (MgModInfo *) calloc (m, sizeof (MgModInfo));
  U8 *info = (U8 *) malloc (m), *qual = (U8 *) malloc (m);
  int *n200 = (int *) calloc ((size_t) rs->nReads + 1, sizeof (int)), *m200 = (int *) calloc ((size_t) rs->nReads + 1, sizeof (int)), *rCount = (int *) calloc (m, sizeof (int));
  int rc = -1;
  if (!mi || !info || !qual || !n200 || !m200 || !rCount) { mgSetErrorText ("-R: out of memory"); goto done; }
  if (s->mi) memcpy (mi, s->mi, m * sizeof (MgModInfo));
  memcpy (info, ms->info, m);
  for (U64 j = 0 ; j < n ; ++j)                                      /* modasm.c:766-773: the last hit of a mod wins rDNApos; bits are only ever set */
    { const U32 ix = index[j];
      info[ix] |= MS_RDNA;
      mi[ix].flags |= RD_REF | rdnaDepthClass (ms->depth[ix]); mi[ix].rDNApos = pos[j];
    }
  for (size_t i = 0 ; i < m ; ++i) qual[i] = (mi[i].flags & (RD_REF | RD_CORE)) == (RD_REF | RD_CORE);      /* fixed from here on: the walk below never sets RD_REF */
  int host = rsHostForced (rs);
  if (!host)
    { MgRsView v; mgRsViewOf (rs, &v);
      const int d = mgRdnaN200Device (&v, qual, n200, m200);
      if (d < 0) goto done;
      host = d;
    }
  if (host) rdnaN200Host (rs, qual, n200, m200);
  U8 *flags = rdnaFlags (s, rs);
  int nRDNAreads = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i)                            /* modasm.c:803-830, in read order: running averages, mods newly flagged by earlier reads */
    { if (m200[i] <= n200[i]) continue;
      const U32 *hit = rs->hit + rs->hitStart[i];
      int lastPos = 0;
      for (int j = n200[i] ; j < m200[i] ; ++j)
        { const U32 h = hit[j] & TOPMASK;
          MgModInfo *q = &mi[h];
          if (q->flags)
            { const int p = q->rDNApos;
              if (q->flags & RD_REF) lastPos = p;
              else if (p > 0 && p < lastPos + 50 && p > lastPos - 50) { q->rDNApos = (rCount[h] * p + lastPos) / (rCount[h] + 1); ++rCount[h]; }
              else q->rDNApos = -1;
            }
          else
            { info[h] |= MS_RDNA; q->flags |= rdnaDepthClass (ms->depth[h]); q->rDNApos = lastPos; rCount[h] = 1; }
        }
      flags[i] |= 1; ++nRDNAreads;
    }
  free (s->mi); s->mi = mi; s->nMi = m;
  memcpy (ms->info, info, m);
  mgModsetHostChanged (ms);
  gRdnaPath = host;
  int nRDNA = 0, nRef = 0, nGoodPos = 0, nRefC = 0, nRefV0 = 0, nRefV1 = 0, nRefM = 0, nOthC = 0, nOthV0 = 0, nOthV1 = 0, nOthM = 0;      /* modasm.c:834-859 */
  for (size_t i = 0 ; i < m ; ++i)
    { const MgModInfo *q = &mi[i];
      if (!q->flags) continue;
      ++nRDNA;
      const int copy0 = (info[i] & 3) == 0;
      if (q->flags & RD_REF)
        { ++nRef;
          if (q->flags & RD_CORE) ++nRefC; else if (q->flags & RD_MULTI) ++nRefM; else if (copy0) ++nRefV0; else ++nRefV1;
        }
      else
        { if (q->flags & RD_CORE) ++nOthC; else if (q->flags & RD_MULTI) ++nOthM; else if (copy0) ++nOthV0; else ++nOthV1;
          if (q->rDNApos > 0) ++nGoodPos;
        }
    }
  if (out)
    { fprintf (out, "total nRDNAreads %d other reads %d\n", nRDNAreads, rs->nReads - nRDNAreads);
      fprintf (out, "total nRDNAmods %d nRDNAref %d other mods %d\n", nRDNA, nRef, (int) m - nRDNA);
      fprintf (out, "  nRefC %d nRefM %d nRefVcopy>0 %d nRefVcopy0 %d\n", nRefC, nRefM, nRefV1, nRefV0);
      fprintf (out, "  nOthC %d nOthM %d nOthVcopy>0 %d nOthVcopy0 %d", nOthC, nOthM, nOthV1, nOthV0);
      fprintf (out, " nGoodPos %d\n", nGoodPos);
    }
  mi = 0; rc = 0;                                                    /* (ModInfo is the set's now) */
done:
  free (mi); free (info); free (qual); free (n200); free (m200); free (rCount);
  return rc;
}

/* the reference sequences' hits in file order: scan with the set's hasher and lookups on the device, as mgRefPaintFile makes them (misses dropped here) */
typedef struct { Modset *ms; U32 *ix; int *pos; U64 n, cap; MgSeedBufs bufs; } RefHitsCtx;
static int refHitsDeviceBatch (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, void *stream)
{
  RefHitsCtx *c = (RefHitsCtx *) v; (void) idBytes; (void) idOff; (void) stream;
  if (!nReads) return 0;
  U64 n = 0;
  if (mgSeedsOfBatch (c->ms, 0, 0, dPacked, total, dOff, nReads, mgSeedGuess (c->ms->hasher->w, total), &c->bufs, &n, 0)) return -1;
  if (!n) return 0;
  U32 *ix = (U32 *) malloc (n * sizeof (U32)), *pf = (U32 *) malloc (n * sizeof (U32));
  int rc = !ix || !pf || mgMemcpyD2H (ix, c->bufs.ix, n * sizeof (U32), 0) || mgMemcpyD2H (pf, c->bufs.posF, n * sizeof (U32), 0) ? -1 : 0;
  if (!rc && c->n + n > c->cap)
    { c->cap = (c->n + n) * 2; c->ix = (U32 *) realloc (c->ix, c->cap * sizeof (U32)); c->pos = (int *) realloc (c->pos, c->cap * sizeof (int));
      if (!c->ix || !c->pos) rc = -1;
    }
  for (U64 j = 0 ; !rc && j < n ; ++j) if (ix[j]) { c->ix[c->n] = ix[j]; c->pos[c->n++] = (int) (pf[j] & MG_POS_MASK); }
  free (ix); free (pf);
  return rc;
}
int mgReadsetRefFlagFile (MgReadset *rs, const char *refFile, FILE *out)      /* modasm.c:752-776, then the above */
{
  gRdnaPath = -1;
  { FILE *f = fopen (refFile, "rb");
    if (!f) { char msg[600]; snprintf (msg, sizeof (msg), "failed to open ref seq file %s", refFile); mgSetErrorText (msg); return -1; }      /* modasm.c:756 */
    fclose (f);
  }
  if (mgIterRequireDevice ()) return -1;
  RefHitsCtx c; memset (&c, 0, sizeof (c)); c.ms = rs->ms;
  U64 nSeq = 0, totLen = 0;
  int rc = mgSeqWalkFile (refFile, refHitsDeviceBatch, 0, &c, 0, 0, &nSeq, &totLen);
  mgSeedBufsFree (&c.bufs);
  if (rc) { if (!mgLastError ()[0]) mgSetErrorText ("-R: failed to read the reference sequence file"); rc = -1; }
  else rc = mgReadsetRefFlagHits (rs, c.ix, c.pos, c.n, out);
  free (c.ix); free (c.pos);
  return rc;
}

int mgReadsetResetBits (MgReadset *rs, int op, FILE *out)          /* modasm.c:864-908 */
{
  gRdnaPath = -1;
  Modset *ms = rs->ms;
  RdnaState *s = rdnaState (rs, 0);
  if (!s || !s->mi) { mgSetErrorText ("-rb: need to run -R first (the reference reads a null ModInfo)"); return -1; }
  if (modsetSyncToHost (ms, 0)) return -1;
  const size_t m = (size_t) ms->max + 1;
  if (s->nMi != m) { mgSetErrorText ("-rb: the modset has changed its size since -R"); return -1; }
  if (op == 3 && rs->nReads < 1) { mgSetErrorText ("-rb 3: the read set is empty (the reference reads read 1)"); return -1; }
  U8 *info = (U8 *) malloc (m);
  int *nc = (int *) calloc (((size_t) rs->nReads + 1) * 4, sizeof (int));
  int rc = -1, n = 0;
  if (!info || !nc) { mgSetErrorText ("-rb: out of memory"); goto done; }
  memcpy (info, ms->info, m);
  const char *line = 0;
  if (op >= 1 && op <= 3)
    { for (size_t i = 0 ; i < m ; ++i)
        if ((s->mi[i].flags & RD_CORE) && !(op == 2 && (info[i] & MS_REPEAT))) { info[i] = (U8) ((info[i] & 0xfc) | 1); ++n; }
        else info[i] &= 0xfc;
      line = op == 1 ? "resetting rDNA core kmers to copy1, rest to copy0:" : op == 2 ? "resetting non-repetitive rDNA core kmers to copy1, rest to copy0:"
                     : "resetting rDNA core kmers not repeated in read 1 to copy1: ";
    }
  if (op == 3)
    { U8 *z = (U8 *) calloc (m, 1);
      for (U64 h = rs->hitStart[1] ; h < rs->hitStart[2] ; ++h)
        { const U32 y = rs->hit[h] & TOPMASK;
          if ((info[y] & 3) != 1) continue;
          if (z[y]) { info[y] &= 0xfc; --n; } else z[y] = 1;
        }
      free (z);
    }
  const int host = rsHostForced (rs);
  if (mgRsCopyTallies (rs, info, host, nc)) goto done;                /* invBuild (modasm.c:907): depth[] is as it was, so only nCopy[] moves */
  memcpy (ms->info, info, m);
  if (rs->nReads) memcpy (rs->nCopy[1], nc + 4, (size_t) rs->nReads * sizeof (int[4]));
  mgModsetHostChanged (ms);
  gRdnaPath = host;
  if (line && out) fprintf (out, "%s %d kept\n", line, n);
  rc = 0;
done:
  free (info); free (nc);
  return rc;
}

/* testMods' gather and rules by loops: per tested mod the count / least / greatest distance per partner in arrays of ms->max + 1 entries that are
   stamped with the tested mod's ordinal, not cleared.  0, or -2 with *badMod where the reference breaks */
static int rdnaTestModsHost (const MgRsView *S, const U32 *tested, U32 nTested, int wantCells, int *res3, int *badLD, int *splitLD, U64 *cellStart, MgLdCell **cellsOut,
                             U64 diag[4], U32 *badMod)
{
  const size_t m = (size_t) S->msMax + 1;
  int maxLen = 0;
  for (U32 r = 1 ; r <= S->nReads ; ++r) if (S->len[r] > maxLen) maxLen = S->len[r];
  int *pos = (int *) malloc ((S->totHit + 1) * sizeof (int));
  for (U32 r = 1 ; r <= S->nReads ; ++r) { int x = 0; for (U64 h = S->hitStart[r] ; h < S->hitStart[r + 1] ; ++h) pos[h] = x += S->dx[h]; }
  U32 *stamp = (U32 *) calloc (m, sizeof (U32)), *touched = (U32 *) malloc (m * sizeof (U32));
  int *cnt = (int *) malloc (m * sizeof (int)), *mn = (int *) malloc (m * sizeof (int)), *mx = (int *) malloc (m * sizeof (int));
  int *start = (int *) calloc ((size_t) maxLen + 2, sizeof (int)), *end = (int *) calloc ((size_t) maxLen + 2, sizeof (int));
  MgLdCell *cells = 0; U64 nCells = 0, capCells = 0;
  int rc = 0, nBigS = 0, nBigE = 0;
  for (U32 t = 0 ; t < nTested && !rc ; ++t)
    { const U32 i = tested[t];
      int extS = 0, extE = 0; U32 nTouched = 0;
      for (U64 v = S->invStart[i] ; v < S->invStart[i + 1] && !rc ; ++v)
        { const U32 r = S->invSpace[v];
          const U64 h0 = S->hitStart[r], h1 = S->hitStart[r + 1];
          U64 f = h0;
          while (f < h1 && (S->hit[f] & TOPMASK) != i) ++f;            /* both visits of a read that holds i twice use the first occurrence */
          const int x = f < h1 ? pos[f] : 0, o = S->len[r] - x - S->w;
          if (f == h1 || o < 0 || x > maxLen || o > maxLen) { rc = -2; *badMod = i; break; }
          const int fwd = (S->hit[f] & TOPBIT) != 0, s = fwd ? x : o, e = fwd ? o : x;
          ++start[s]; ++end[e];
          if (s + 1 > extS) extS = s + 1;
          if (e + 1 > extE) extE = e + 1;
          for (U64 h = h0 ; h < h1 ; ++h)
            { const U32 y = S->hit[h] & TOPMASK;
              if (h == f || !mgRdnaCheckMod (S->info[y])) continue;
              const int d = fwd ? pos[h] - x : x - pos[h];
              if (stamp[y] != t + 1) { stamp[y] = t + 1; touched[nTouched++] = y; cnt[y] = 0; mn[y] = mx[y] = d; }
              ++cnt[y];
              if (d < mn[y]) mn[y] = d;
              if (d > mx[y]) mx[y] = d;
            }
        }
      if (!rc && ((extS > MG_RDNA_CLEARED && ++nBigS > 1) || (extE > MG_RDNA_CLEARED && ++nBigE > 1))) { rc = -3; *badMod = i; }
      if (!rc)
        { for (int k = extS - 1 ; k-- > 0 ; ) start[k] += start[k + 1];      /* modasm.c:651-654 */
          for (int k = extE - 1 ; k-- > 0 ; ) end[k] += end[k + 1];
          qsort (touched, nTouched, sizeof (U32), rsU32Cmp);
          if (wantCells && nCells + nTouched > capCells) { capCells = (nCells + nTouched) * 2 + 64; cells = (MgLdCell *) realloc (cells, capCells * sizeof (MgLdCell)); }
          for (U32 q = 0 ; q < nTouched ; ++q)
            { const U32 y = touched[q];
              MgLdCell c; c.m = y;
              if (mgRdnaLdRule (cnt[y], mn[y], mx[y], start, extS, end, extE, (int) S->depth[y], S->run, &c)) { rc = -2; *badMod = i; break; }
              diag[3] += (U64) cnt[y];
              if (c.flags & MG_LD_GOOD) ++res3[3 * (size_t) t];
              if (c.flags & MG_LD_MOD2) ++res3[3 * (size_t) t + 1];
              if (c.flags & MG_LD_SPLIT) { ++res3[3 * (size_t) t + 2]; ++splitLD[y]; }
              if (c.flags & MG_LD_BAD_M) ++badLD[y];
              if (c.flags & MG_LD_BAD_I) ++badLD[i];
              if (wantCells) cells[nCells++] = c;
            }
          if (cellStart) cellStart[t + 1] = wantCells ? nCells : 0;
        }
      memset (start, 0, (size_t) (extS > 0 ? extS : 1) * sizeof (int)); memset (end, 0, (size_t) (extE > 0 ? extE : 1) * sizeof (int));
    }
  free (pos); free (stamp); free (touched); free (cnt); free (mn); free (mx); free (start); free (end);
  if (rc) { free (cells); return rc; }
  diag[0] = nTested ? 1 : 0;
  *cellsOut = cells;
  return 0;
}

/* the closing loop of testMods (modasm.c:708-740) over ModInfo: the copy-0 resets into info[], the "YY-TEST" lines into yFile (0: none); the misleading
   braces at RUN 4 and 8 -- "BADLD" printed for, and copy 0 given to, EVERY mod -- are kept */
static void rdnaTestModsClose (const MgModInfo *mi, size_t m, const U16 *depth, U8 *info, int run, FILE *yFile, int zero[3])
{
  zero[0] = zero[1] = zero[2] = 0;
  for (size_t i = 0 ; i < m ; ++i)
    { const MgModInfo *q = &mi[i];
      const int d = depth[i];
#define RD_BADLD() do { if (yFile) fprintf (yFile, "BADLD %d depth %d nBadLD %d nSplitLD %d\n", (int) i, d, q->nBadLD, q->nSplitLD); info[i] &= 0xfc; ++zero[2]; } while (0)
      if ((q->nGood || q->nMod2) && yFile) fprintf (yFile, "TEST %d depth %d nGood %d nMod2 %d nBadLD %d nSplit %d\n", (int) i, d, q->nGood, q->nMod2, q->nBadLD, q->nSplit);
      if (q->nGood < q->nMod2) { info[i] &= 0xfc; ++zero[0]; }
      if (q->nSplit > 10) { info[i] &= 0xfc; ++zero[1]; }
      if ((run == 2 || run == 6) && (q->nBadLD > 20 || q->nSplitLD > 10)) RD_BADLD ();
      if (run == 3 || run == 7)
        { if (q->nMod2 > 25) { info[i] &= 0xfc; ++zero[0]; }
          if (q->nSplit) { info[i] &= 0xfc; ++zero[1]; }
          if (q->nBadLD > 10) RD_BADLD ();
        }
      if (run == 4 || run == 8)
        { if (q->nBadLD > 6 && q->nSplit) { info[i] &= 0xfc; ++zero[1]; }
          RD_BADLD ();
        }
#undef RD_BADLD
    }
}

int mgReadsetTestMods (MgReadset *rs, int minDepth, int maxDepth, FILE *yFile, FILE *zFile, FILE *out)      /* modasm.c:595-748 */
{
  gRdnaPath = -1; memset (gRdnaDiag, 0, sizeof (gRdnaDiag)); memset (gRdnaGrid, 0, sizeof (gRdnaGrid));
  Modset *ms = rs->ms;
  RdnaState *s = rdnaState (rs, 0);
  if (!s || !s->mi) { mgSetErrorText ("need to run -R first"); return -1; }      /* modasm.c:609 */
  if (modsetSyncToHost (ms, 0)) return -1;
  const size_t m = (size_t) ms->max + 1;
  char msg[240];
  if (s->nMi != m) { mgSetErrorText ("-T: the modset has changed its size since -R"); return -1; }
  if (!rs->invStart || !rs->invSpace) { mgSetErrorText ("-T: the read set has no inverse lists (nothing was read into it)"); return -1; }
  if (rs->invStart[m] > rs->totHit) { mgSetErrorText ("-T: the depths of the mods add up to more than the hits of the reads: the inverse lists do not fit (modasm.c:265-270)"); return -1; }
  U32 *tested = (U32 *) malloc (m * sizeof (U32)), *partner = (U32 *) malloc (m * sizeof (U32));
  U32 nTested = 0, nPartner = 0; U64 visits = 0, walked = 0;      /* walked: the hits of the visited reads, a bound of the partner occurrences */
  int rc = 0;
  for (size_t i = 0 ; i < m && !rc ; ++i)                            /* modasm.c:614-615; the partners are the mods that pass checkMod */
    { if (!mgRdnaCheckMod (ms->info[i])) continue;
      partner[nPartner++] = (U32) i;
      const int d = ms->depth[i];
      if (d < minDepth || d >= maxDepth) continue;
      const U64 a = rs->invStart[i], e = rs->invStart[i + 1];
      if (d == 0 || d == 0xffff || e - a != (U64) d || e > rs->totHit)
        { snprintf (msg, sizeof (msg), "-T: tested mod %u has depth %d and a list of %llu reads (a mod of depth 0 or 65535 has no list: modasm.c:266,617)", (U32) i, d, (unsigned long long) (e - a));
          mgSetErrorText (msg); rc = -1; break; }
      for (U64 v = a ; v < e ; ++v)
        { if (rs->invSpace[v] < 1 || rs->invSpace[v] > (U32) rs->nReads) { mgSetErrorText ("-T: an inverse list names a read that is not in the set"); rc = -1; break; }
          walked += rs->hitStart[rs->invSpace[v] + 1] - rs->hitStart[rs->invSpace[v]];
        }
      tested[nTested++] = (U32) i; visits += e - a;
    }
  if (!rc && !nTested) { mgSetErrorText ("-T: no mod tested (the reference dies at the end of such a call: arrayDestroy (0), modasm.c:746)"); rc = -1; }
  const int run = s->run + 1;
  int *res3 =(int *) calloc ((size_t) nTested * 3 + 1, sizeof (int)), *badLD = (int *) calloc (m, sizeof (int)), *splitLD = (int *) calloc (m, sizeof (int));
  U64 *cellStart = (U64 *) calloc ((size_t) nTested + 2, sizeof (U64));
  MgLdCell *cells = 0;
  MgModInfo *mi = (MgModInfo *) malloc (m * sizeof (MgModInfo));
  U8 *info = (U8 *) malloc (m);
  int *nc = (int *) calloc (((size_t) rs->nReads + 1) * 4, sizeof (int));
  /* a call that walks fewer than MG_RDNA_DEVICE_MIN hits is done by the host loops before the set's arrays have reached the device (2.3 ms
     against 1.6 ms at 2 x 10^4 occurrences, 2.8 ms against 100 ms at 10^8); MODGPU_READSET_HOST=0 sends every call to the device */
  int host = rsHostForced (rs) || (walked < MG_RDNA_DEVICE_MIN && mgKnobs ()->readsetHost != 0);
  U32 badMod = 0;
  if (!rc)
    { MgRsView S; mgRsViewOf (rs, &S); S.run = run;
      const MgKnobs *kn = mgKnobs ();
      const U32 batch = kn->testModsBatch != MG_KNOB_UNSET && kn->testModsBatch > 0 ? (U32) kn->testModsBatch : 0;
      if (!host)
        { rc = mgRdnaTestModsDevice (&S, tested, nTested, partner, nPartner, batch, zFile != 0, res3, badLD, splitLD, cellStart, &cells, gRdnaDiag, gRdnaGrid, &badMod);
          if (rc == 1) { host = 1; rc = 0; memset (res3, 0, ((size_t) nTested * 3 + 1) * sizeof (int)); memset (badLD, 0, m * sizeof (int)); memset (splitLD, 0, m * sizeof (int)); memset (gRdnaDiag, 0, sizeof (gRdnaDiag)); memset (gRdnaGrid, 0, sizeof (gRdnaGrid)); }
        }
      if (host && !rc) rc = rdnaTestModsHost (&S, tested, nTested, zFile != 0, res3, badLD, splitLD, cellStart, &cells, gRdnaDiag, &badMod);
      if (rc == -2)
        { snprintf (msg, sizeof (msg), "-T: tested mod %u: a visit counts before its array (len - x - w < 0) or a distance is looked up beyond it (modasm.c:630,664,689); w > k?", badMod);
          mgSetErrorText (msg); rc = -1; }
      if (rc == -3)
        { snprintf (msg, sizeof (msg), "-T: tested mod %u is the second whose count array passes 20000 cells: the reference clears only the first 20000 between tested mods and counts on stale cells (modasm.c:619-620, array.c:103)", badMod);
          mgSetErrorText (msg); rc = -1; }
    }
  int zero[3];
  if (!rc)
    { memcpy (mi, s->mi, m * sizeof (MgModInfo)); memcpy (info, ms->info, m);
      for (size_t i = 0 ; i < m ; ++i) { mi[i].nGood = mi[i].nMod2 = mi[i].nSplit = 0; mi[i].nBadLD = badLD[i]; mi[i].nSplitLD = splitLD[i]; }      /* modasm.c:610-611 */
      for (U32 t = 0 ; t < nTested ; ++t) { MgModInfo *q = &mi[tested[t]]; q->nGood = res3[3 * (size_t) t]; q->nMod2 = res3[3 * (size_t) t + 1]; q->nSplit = res3[3 * (size_t) t + 2]; }
      rdnaTestModsClose (mi, m, ms->depth, info, run, 0, zero);
      if (mgRsCopyTallies (rs, info, host, nc)) rc = -1;                 /* invBuild (modasm.c:744): nCopy[] after the copy-0 resets */
    }
  if (!rc)
    { if (zFile)
        for (U32 t = 0 ; t < nTested ; ++t)
          for (U64 c = cellStart[t] ; c < cellStart[t + 1] ; ++c)
            fprintf (zFile, "i %d depth %d m %d depth %d %c count %d min %d at %d max %d at %d\n", (int) tested[t], (int) ms->depth[tested[t]], (int) cells[c].m, (int) ms->depth[cells[c].m],
                     (cells[c].flags & MG_LD_PLUS) ? '+' : '-', cells[c].n, cells[c].vmin, cells[c].xmin, cells[c].vmax, cells[c].xmax);
      memcpy (info, ms->info, m);
      rdnaTestModsClose (mi, m, ms->depth, info, run, yFile, zero);
      memcpy (ms->info, info, m);
      { MgModInfo *old = s->mi; s->mi = mi; mi = old; }
      if (rs->nReads) memcpy (rs->nCopy[1], nc + 4, (size_t) rs->nReads * sizeof (int[4]));
      s->run = run;
      mgModsetHostChanged (ms);
      gRdnaPath = host; gRdnaDiag[1] = nTested; gRdnaDiag[2] = visits;
      if (out) fprintf (out, "RUN %d tested %d mods and zeroed %d bad>good %d split %d LD\n", run, (int) nTested, zero[0], zero[1], zero[2]);
    }
  free (tested); free (partner); free (res3); free (badLD); free (splitLD); free (cellStart); free (cells); free (mi); free (info); free (nc);
  return rc;
}
