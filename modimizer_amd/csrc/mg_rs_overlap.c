/* mg_rs_overlap.c — modasm -o1 / -o2 / -b / -c over a read set: findOverlaps (modasm.c:314-418) and its callers markBadReads (1266-1322), markContained (1370-1394).
 * findOverlaps (x) splits into a record per partner y that depends on the two hit lists and on info[] / depth[] alone -- made for a batch of queries
 * at once, on the device (mg_overlap.hip) or by the loops below -- and a replay that reads and writes the reads' `bad` in the order of the calls
 * (ovlReplay).  The host loops stamp their per-mod and per-read arrays with the query's serial number where the reference clears them per call. */
#include "mg_readset_int.h"

static __thread int gOverlapsPath = -1;
static __thread U64 gOverlapsDiag[4];
int mgReadsetOverlapsPath (void) { return gOverlapsPath; }
void mgReadsetOverlapsDiag (U64 out4[4]) { memcpy (out4, gOverlapsDiag, sizeof (gOverlapsDiag)); }

enum { BAD_REPEAT = 1, BAD_ORDER10 = 2, BAD_ORDER1 = 4, BAD_NOMATCH = 8, BAD_LOWHIT = 16, BAD_LOWCOPY1 = 32 };      /* modasm.c:38-45 */
enum { OVL_PLUS = 1, OVL_CONTAINED = 2, OVL_SKIPPED = 4 };

typedef struct { U32 iy, nHit; U64 first; } OvlCand;
typedef struct {
  U32 *modStamp, *readStamp, *readSlot; U16 *modJ;      /* hmap / omap of modasm.c:317-321, valid where the stamp is the query's */
  U32 stamp;
  OvlCand *cand; U64 capCand;
  int64_t *xPos; U64 capPos;
} OvlHost;

static int ovlCandCmp (const void *a, const void *b)     /* nHit descending, equal nHit in arrival order: what the reference's sort by nHit alone leaves (glibc's qsort is a stable merge sort) */
{
  const OvlCand *x = (const OvlCand *) a, *y = (const OvlCand *) b;
  if (x->nHit != y->nHit) return x->nHit > y->nHit ? -1 : 1;
  return x->first < y->first ? -1 : x->first > y->first;
}

/* the record of (x, y): modasm.c:359-390 in one walk of y's hits.  Both order tests are counted (they depend on the sequence of matches alone), the
   majority picks one afterwards */
static void ovlPairHost (const MgReadset *rs, const OvlHost *H, U32 x, U32 y, MgOvlRec *r)
{
  const U64 ax = rs->hitStart[x], ay = rs->hitStart[y], ey = rs->hitStart[y + 1];
  U32 nPlus = 0, nMinus = 0, nLess = 0, nGreater = 0, lastLess = 0, lastGreater = (U32) rs->nHit[x];
  int64_t yPos = 0, firstDiff = 0, lastDiff = 0; int any = 0;
  for (U64 h = ay ; h < ey ; ++h)
    { const U32 hy = rs->hit[h], m = hy & TOPMASK;
      yPos += rs->dx[h];
      if (H->modStamp[m] != H->stamp) continue;
      const U32 ihx = H->modJ[m];                                    /* j + 1 */
      if ((hy & TOPBIT) == (rs->hit[ax + ihx - 1] & TOPBIT)) ++nPlus; else ++nMinus;
      lastDiff = H->xPos[ihx] - yPos;
      if (!any) { firstDiff = lastDiff; any = 1; }
      if (ihx < lastLess) ++nLess;
      if (ihx > lastGreater) ++nGreater;
      lastLess = lastGreater = ihx;
    }
  r->nBadOrder = r->nBadFlip = r->flags = 0;
  if (nPlus > nMinus)
    { r->flags = OVL_PLUS; r->nBadFlip = (U16) nMinus; r->nBadOrder = (U16) nLess; nPlus -= nLess;
      if (firstDiff < 0 && !((int64_t) rs->len[x] - lastDiff > (int64_t) rs->len[y])) r->flags |= OVL_CONTAINED;
    }
  else if (nMinus && !nPlus) { r->nBadOrder = (U16) nGreater; nMinus -= nGreater; }      /* (isContained cannot be set here: modasm.c:382,386) */
  r->nPlus = (U16) nPlus; r->nMinus = (U16) nMinus;
}

typedef struct { MgOvlRec *recs; U64 n, cap; } OvlRecs;
static MgOvlRec *ovlRecsRoom (OvlRecs *R, U64 more)
{
  if (R->n + more > R->cap) { R->cap = (R->n + more) * 2 + 64; R->recs = (MgOvlRec *) realloc (R->recs, R->cap * sizeof (MgOvlRec)); }
  return R->recs ? R->recs + R->n : 0;
}

static int ovlBatchHost (const MgReadset *rs, OvlHost *H, const U32 *queries, U32 nq, U32 *nRepeat, U64 *start, MgOvlRec **recsOut, U64 diag[4])
{
  const Modset *ms = rs->ms;
  OvlRecs R = { 0, 0, 0 };
  for (U32 q = 0 ; q < nq ; ++q)
    { const U32 x = queries[q];
      const U64 ax = rs->hitStart[x], nx = rs->hitStart[x + 1] - ax;
      ++H->stamp;
      if (nx + 1 > H->capPos) { H->capPos = nx + 1; H->xPos = (int64_t *) realloc (H->xPos, H->capPos * sizeof (int64_t)); if (!H->xPos) return -1; }
      U64 nCand = 0, walked = 0; U32 rep = 0;
      H->xPos[0] = 0;
      for (U64 j = 0 ; j < nx ; ++j)
        { const U32 m = rs->hit[ax + j] & TOPMASK;
          H->xPos[j + 1] = H->xPos[j] + rs->dx[ax + j];
          if ((ms->info[m] & 3) != 1) continue;
          if (H->modStamp[m] == H->stamp) { ++rep; continue; }
          H->modStamp[m] = H->stamp; H->modJ[m] = (U16) (j + 1);
          for (U64 k = rs->invStart[m] ; k < rs->invStart[m + 1] ; ++k, ++walked)
            { const U32 y = rs->invSpace[k];
              if (H->readStamp[y] != H->stamp)
                { H->readStamp[y] = H->stamp; H->readSlot[y] = (U32) nCand;
                  if (nCand == H->capCand) { H->capCand = H->capCand ? H->capCand * 2 : 256; H->cand = (OvlCand *) realloc (H->cand, H->capCand * sizeof (OvlCand)); if (!H->cand) return -1; }
                  H->cand[nCand].iy = y; H->cand[nCand].nHit = 0; H->cand[nCand].first = walked; ++nCand;
                }
              ++H->cand[H->readSlot[y]].nHit;
            }
        }
      nRepeat[q] = rep; start[q] = R.n; diag[1] += walked;
      qsort (H->cand, nCand, sizeof (OvlCand), ovlCandCmp);
      U64 keep = 0; while (keep < nCand && H->cand[keep].nHit >= 3) ++keep;
      MgOvlRec *r = ovlRecsRoom (&R, keep + 1);
      if (!r) return -1;
      for (U64 c = 0 ; c < keep ; ++c) { r[c].iy = H->cand[c].iy; r[c].nHit = (U16) H->cand[c].nHit; ovlPairHost (rs, H, x, r[c].iy, &r[c]); }
      R.n += keep; diag[2] += keep;
    }
  start[nq] = R.n;
  if (!R.recs) R.recs = (MgOvlRec *) malloc (sizeof (MgOvlRec));
  *recsOut = R.recs;
  return 0;
}

/* findOverlaps (x, level) from x's records: what depends on the flags as they are now (modasm.c:336,358,391-415).  A skipped record is left as -b / -c
   see it: zero counts and flags */
static void ovlReplay (MgReadset *rs, U32 x, U32 nRepeat, MgOvlRec *recs, U64 n, int level, FILE *out)
{
  if (nRepeat) rs->bad[x] |= BAD_REPEAT;
  int nGood = 0, nBad = 0;
  for (U64 i = 0 ; i < n ; ++i)
    { MgOvlRec *o = &recs[i];
      if (rs->bad[o->iy]) { o->nBadOrder = o->nBadFlip = 0; o->flags = OVL_SKIPPED; continue; }
      const int isBad = o->nBadOrder || o->nBadFlip;
      if (isBad) ++nBad; else ++nGood;
      if (level > 1 && out)
        fprintf (out, "RH\t%u\tlen %d\t%s\t+ %d\t- %d\tbadOrder %d\t%s\n", o->iy, rs->len[o->iy], isBad ? "BAD" : "GOOD", (int) o->nPlus, (int) o->nMinus, (int) o->nBadOrder,
                 (o->flags & OVL_CONTAINED) ? "CONTAINED" : "OVERLAP");
    }
  if (!nGood && !nBad)
    { rs->bad[x] |= BAD_NOMATCH;
      if (rs->nHit[x] < 10) rs->bad[x] |= BAD_LOWHIT;
      else if (rs->nCopy[x][1] < 10) rs->bad[x] |= BAD_LOWCOPY1;
    }
  if (level > 0 && out)
    { fprintf (out, "RR %6u\tlen %d\tnHit %3d\tnMiss %3d\t", x, rs->len[x], rs->nHit[x], rs->nMiss[x]);
      fprintf (out, "nCpy %d %d %d %d\t", rs->nCopy[x][0], rs->nCopy[x][1], rs->nCopy[x][2], rs->nCopy[x][3]);
      fprintf (out, "nRepeatMod %d\tnGood %4d\tnBad %4d\n", (int) nRepeat, nGood, nBad);
    }
}

void mgOverlapsFree (MgOverlaps *res)
{
  if (!res) return;
  free (res->start); free (res->iy); free (res->nHit); free (res->nBadOrder); free (res->nBadFlip); free (res->flags);
  memset (res, 0, sizeof (*res));
}

typedef void (*OvlEach) (void *ctx, U32 x, const MgOvlRec *recs, U64 n);

/* the queries in the order given: checks, batches by the candidate budget, per batch the records (device or host loops), then the replay of its queries
   in order before the next batch's records are made -- the records do not read the flags, so only the replay is ordered */
static int ovlDrive (MgReadset *rs, const U32 *reads, U32 n, int level, FILE *out, MgOverlaps *res, OvlEach each, void *ctx)
{
  Modset *ms = rs->ms;
  const U32 nReads = (U32) rs->nReads;
  if (res) memset (res, 0, sizeof (*res));
  if (modsetSyncToHost (ms, 0)) return -1;
  if (!rs->invStart || !rs->invSpace) { mgSetErrorText ("overlaps: the read set has no inverse lists (nothing was read into it)"); return -1; }
  for (U32 i = 1 ; i <= nReads ; ++i)
    if (rs->nHit[i] > 65534 || rs->hitStart[i + 1] - rs->hitStart[i] > 65534)
      { char msg[160]; snprintf (msg, sizeof (msg), "overlaps: read %u has more than 65534 hits (the reference's 16-bit hit numbers wrap there)", i); mgSetErrorText (msg); return -1; }
  U64 *bound = (U64 *) malloc (((size_t) n + 1) * sizeof (U64));      /* per query: its candidates, repeats' lists counted too */
  U64 maxBound = 0;
  for (U32 q = 0 ; q < n ; ++q)
    { const U32 x = reads[q];
      if (x < 1 || x > nReads)
        { char msg[160]; snprintf (msg, sizeof (msg), "overlaps: read %u is not in the read set (reads 1 .. %u)", x, nReads); mgSetErrorText (msg); free (bound); return -1; }
      U64 b = 0;
      for (U64 h = rs->hitStart[x] ; h < rs->hitStart[x + 1] ; ++h)
        { const U32 m = rs->hit[h] & TOPMASK;
          if ((ms->info[m] & 3) != 1) continue;
          if (ms->depth[m] == 0xffff)
            { char msg[200]; snprintf (msg, sizeof (msg), "overlaps: copy-1 mod %u of read %u has a saturated depth and so no inverse list (modasm.c:266,338)", m, x); mgSetErrorText (msg); free (bound); return -1; }
          b += rs->invStart[m + 1] - rs->invStart[m];
        }
      bound[q] = b; if (b > maxBound) maxBound = b;
    }
  const MgKnobs *kn = mgKnobs ();
  int host = rsHostForced (rs) || maxBound >= 0x7fffffffull;
  MgOvlDev *dev = 0;
  if (!host)
    { MgRsView v; mgRsViewOf (rs, &v);
      const int rc = mgOvlDevOpen (&dev, &v);
      if (rc < 0) { free (bound); return -1; }
      host = rc;
    }
  U64 budget = kn->overlapCands != MG_KNOB_UNSET && kn->overlapCands > 0 ? (U64) kn->overlapCands : host ? (U64) 1 << 24 : mgOvlDevCandBudget ();
  if (budget > 0x7fffffffull) budget = 0x7fffffffull;
  OvlHost H; memset (&H, 0, sizeof (H));
  MgOverlaps R; memset (&R, 0, sizeof (R));
  U64 capRes = 0, nRes = 0;
  int rc = 0;
  if (res) { R.n = n; R.start = (U64 *) calloc ((size_t) n + 1, sizeof (U64)); }
  U32 *nRepeat = 0; U64 *start = 0; U32 capQ = 0;
  for (U32 q0 = 0 ; q0 < n && !rc ; )
    { U32 q1 = q0; U64 cands = 0, hits = 0;
      while (q1 < n && (q1 == q0 || (cands + bound[q1] <= budget && hits + (U64) rs->nHit[reads[q1]] < 0x7fffffffull && q1 - q0 < (1u << 24))))
        { cands += bound[q1]; hits += (U64) rs->nHit[reads[q1]]; ++q1; }
      const U32 nq = q1 - q0;
      if (nq > capQ) { capQ = nq; nRepeat = (U32 *) realloc (nRepeat, (size_t) capQ * sizeof (U32)); start = (U64 *) realloc (start, ((size_t) capQ + 1) * sizeof (U64)); }
      MgOvlRec *recs = 0;
      if (!host)
        { const int d = mgOvlDevBatch (dev, reads + q0, nq, nRepeat, start, &recs, gOverlapsDiag);
          if (d < 0) { rc = -1; break; }
          if (d > 0) { host = 1; mgOvlDevClose (dev); dev = 0; }      /* no room for this batch: the host loops, from here on */
        }
      if (host)
        { if (!H.modStamp)
            { H.modStamp = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32)); H.modJ = (U16 *) calloc ((size_t) ms->max + 1, sizeof (U16));
              H.readStamp = (U32 *) calloc ((size_t) nReads + 1, sizeof (U32)); H.readSlot = (U32 *) calloc ((size_t) nReads + 1, sizeof (U32));
              if (!H.modStamp || !H.modJ || !H.readStamp || !H.readSlot) { mgSetErrorText ("overlaps: out of memory"); rc = -1; break; }
            }
          if (ovlBatchHost (rs, &H, reads + q0, nq, nRepeat, start, &recs, gOverlapsDiag)) { mgSetErrorText ("overlaps: out of memory"); rc = -1; break; }
        }
      ++gOverlapsDiag[0];
      for (U32 q = 0 ; q < nq ; ++q)
        { const U32 x = reads[q0 + q];
          MgOvlRec *r = recs + start[q]; const U64 nr = start[q + 1] - start[q];
          ovlReplay (rs, x, nRepeat[q], r, nr, level, out);
          if (each) each (ctx, x, r, nr);
          if (res)
            { if (nRes + nr > capRes)
                { capRes = (nRes + nr) * 2 + 64;
                  R.iy = (U32 *) realloc (R.iy, capRes * sizeof (U32)); R.nHit = (U16 *) realloc (R.nHit, capRes * sizeof (U16)); R.nBadOrder = (U16 *) realloc (R.nBadOrder, capRes * sizeof (U16));
                  R.nBadFlip = (U16 *) realloc (R.nBadFlip, capRes * sizeof (U16)); R.flags = (U8 *) realloc (R.flags, capRes * sizeof (U8));
                }
              for (U64 i = 0 ; i < nr ; ++i)
                { R.iy[nRes + i] = r[i].iy; R.nHit[nRes + i] = r[i].nHit; R.nBadOrder[nRes + i] = r[i].nBadOrder; R.nBadFlip[nRes + i] = r[i].nBadFlip; R.flags[nRes + i] = (U8) r[i].flags; }
              nRes += nr; R.start[q0 + q + 1] = nRes;
            }
        }
      free (recs);
      q0 = q1;
    }
  if (dev) mgOvlDevClose (dev);
  free (H.modStamp); free (H.modJ); free (H.readStamp); free (H.readSlot); free (H.cand); free (H.xPos);
  free (nRepeat); free (start); free (bound);
  if (rc) { mgOverlapsFree (&R); return -1; }
  if (res) *res = R;
  gOverlapsPath = host;
  return 0;
}

int mgReadsetFindOverlaps (MgReadset *rs, const U32 *reads, U32 n, int level, FILE *out, MgOverlaps *res)
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  return ovlDrive (rs, reads, n, level, out, res, 0, 0);
}

int mgReadsetOverlapStats (MgReadset *rs, U32 d, FILE *out)         /* modasm.c:1586-1592 */
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  if (!d) { mgSetErrorText ("overlaps: -o2 0 never ends in the reference; the step is at least 1"); return -1; }
  const U32 n = (U32) rs->nReads / d;
  U32 *reads = (U32 *) malloc (((size_t) n + 1) * sizeof (U32));
  for (U32 i = 0 ; i < n ; ++i) reads[i] = (i + 1) * d;
  const int rc = ovlDrive (rs, reads, n, 1, out, 0, 0, 0);
  free (reads);
  return rc;
}

typedef struct { int *badList, *nBad, *lBad; } OvlMarkBad;
static void ovlMarkBadEach (void *v, U32 ix, const MgOvlRec *recs, U64 n)      /* modasm.c:1283-1289 */
{
  OvlMarkBad *b = (OvlMarkBad *) v;
  for (U64 i = 0 ; i < n ; ++i)
    if (recs[i].nBadFlip || recs[i].nBadOrder)
      { const U32 iy = recs[i].iy;
        ++b->nBad[iy];
        if (b->nBad[iy] < 10 && b->lBad[ix] < 10) b->badList[10 * (size_t) ix + b->lBad[ix]++] = (int) iy;
      }
}
static void ovlDropBad (const MgReadset *rs, OvlMarkBad *b)          /* modasm.c:1299-1302 */
{
  for (int ix = 1 ; ix <= rs->nReads ; ++ix)
    for (int i = b->lBad[ix] ; i-- ; )
      if (rs->bad[b->badList[10 * (size_t) ix + i]]) b->badList[10 * (size_t) ix + i] = b->badList[10 * (size_t) ix + --b->lBad[ix]];
}

int mgReadsetMarkBadReads (MgReadset *rs, FILE *out)                /* modasm.c:1266-1322 */
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  const int n = rs->nReads;
  memset (rs->bad, 0, (size_t) n + 1);
  OvlMarkBad b;
  b.badList = (int *) calloc (((size_t) n + 1) * 10, sizeof (int)); b.nBad = (int *) calloc ((size_t) n + 1, sizeof (int)); b.lBad = (int *) calloc ((size_t) n + 1, sizeof (int));
  U32 *reads = (U32 *) malloc (((size_t) n + 1) * sizeof (U32));
  for (int i = 0 ; i < n ; ++i) reads[i] = (U32) i + 1;
  const int rc = ovlDrive (rs, reads, (U32) n, 0, 0, 0, ovlMarkBadEach, &b);
  free (reads);
  if (!rc)
    { int N = 0;
      for (int ix = 1 ; ix <= n ; ++ix) if (b.nBad[ix] >= 10) { rs->bad[ix] |= BAD_ORDER10; ++N; b.lBad[ix] = 0; }
      if (out) fprintf (out, "MB  %d with >=10 bad overlaps\n", N);
      ovlDropBad (rs, &b);
      N = 0;
      for (int ix = 1 ; ix <= n ; ++ix) if (b.lBad[ix] >= 2) { rs->bad[ix] |= BAD_ORDER1; ++N; b.lBad[ix] = 0; }
      if (out) fprintf (out, "MB  %d with multiple bad overlaps\n", N);
      ovlDropBad (rs, &b);
      N = 0;
      for (int ix = 1 ; ix <= n ; ++ix) if (b.lBad[ix] > 0) { rs->bad[ix] |= BAD_ORDER1; ++N; b.lBad[ix] = 0; }
      if (out) fprintf (out, "MB  %d with single bad overlaps\n", N);
    }
  free (b.badList); free (b.nBad); free (b.lBad);
  return rc;
}

typedef struct { MgReadset *rs; } OvlContained;
static void ovlContainedEach (void *v, U32 ix, const MgOvlRec *recs, U64 n)    /* modasm.c:1382-1389 */
{
  MgReadset *rs = ((OvlContained *) v)->rs;
  int maxHit = 0;
  for (U64 i = 0 ; i < n ; ++i)
    { if (recs[i].iy == ix) continue;
      if (!(recs[i].flags & OVL_CONTAINED) || (int) recs[i].nHit <= maxHit) continue;
      rs->contained[ix] = (int) recs[i].iy; maxHit = recs[i].nHit;
    }
}

int mgReadsetMarkContained (MgReadset *rs, FILE *out)               /* modasm.c:1370-1394 */
{
  gOverlapsPath = -1; memset (gOverlapsDiag, 0, sizeof (gOverlapsDiag));
  const int n = rs->nReads;
  /* a read that is bad when its turn comes is not looked at (modasm.c:1380); a read's own flags are only ever set by its own turn, so which reads
     those are is known now */
  U32 *reads = (U32 *) calloc ((size_t) n + 1, sizeof (U32)); U32 nq = 0;
  for (int i = 1 ; i <= n ; ++i) if (!rs->bad[i]) reads[nq++] = (U32) i;
  OvlContained c; c.rs = rs;
  const int rc = ovlDrive (rs, reads, nq, 0, 0, 0, ovlContainedEach, &c);
  if (!rc)
    { int nContained = 0, nNot = 0; U64 totLen = 0;
      for (U32 q = 0 ; q < nq ; ++q) { const U32 ix = reads[q]; if (rs->contained[ix]) ++nContained; else { ++nNot; totLen += (U64) rs->len[ix]; } }
      if (out) fprintf (out, "MC  found %d contained reads, leaving %d not contained, av length %.1f\n", nContained, nNot, nNot ? totLen / (double) nNot : 0.);
    }
  free (reads);
  return rc;
}
