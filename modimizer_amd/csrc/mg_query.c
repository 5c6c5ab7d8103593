/* mg_query.c — modmap's queryProcess (modmap.c:188-281) over a batch that is on the device.
 * Scan, lookup, the tallies of the "Q" line and the chaining into "M" blocks all run on the device (mg_chain.hip: one lane per
 * read); the lines are formatted from a few integers per read and block (mg_queryout.c).  The long way -- seed lists back on the
 * host, tallies and chaining here, restated with the reference's quirks -- takes a batch with a read of more blocks than the chain
 * kernel keeps, and every batch under -v.
 */
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"
#include "mg_internal.h"

/* one end-of-block test, modmap.c:232-241 (repeated at :245-254 without the "no block" clause) */
static bool blockEnds (const MgReference *ref, U32 loc, U32 loc0, U32 locN, U32 i0, U32 iN, bool withUnset)
{
  if (withUnset && !loc0) return true;
  if (ref->id[loc] != ref->id[loc0]) return true;
  bool end = false;
  if (loc0 < locN)
    { if (loc < locN) end = true;
      int dd = (int) (locN - loc0 - iN + i0); if (dd > 50 || dd < -50) end = true;
    }
  else if (loc0 > locN)
    { if (loc > locN) end = true;
      int dd = (int) (loc0 - locN - iN + i0); if (dd > 50 || dd < -50) end = true;
    }
  return end;
}

static void printM (const MgReference *ref, FILE *out, const char *name, const U32 *seedPos,
                    U32 i0, U32 iN, U32 loc0, U32 locN, int n1, int n2, int copy1)
{
  fprintf (out, "M\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d %d\t%.2f\t%.2f\n",
           name, (int) seedPos[i0], (int) seedPos[iN], (int) (seedPos[iN] - seedPos[i0]),
           ref->names[ref->id[loc0]], (int) ref->offset[loc0], (int) ref->offset[locN],
           n1, n2, (n1 + n2) / (double) ((locN > loc0) ? (locN - loc0) : (loc0 - locN)),
           n1 / (double) copy1);
}

static int gVerbose = 0;                          /* modmap's global isVerbose (modmap.c:23), toggled by -v (modmap.c:348) */
void mgSetVerbose (int on) { gVerbose = on != 0; }
int mgQueryVerbose (void) { return gVerbose; }

/* the long way: seed lists back on the host, tallies and chaining here (used when a read has more blocks
 * than the device kernel keeps) */
static int queryProcessHostChain (MgReference *ref, MgDevBatch *b, const int64_t *offsets, int nReads,
                                  const char **names, FILE *out)
{
  Modset *ms = ref->ms;
  U64 n = 0;
  MgSeedBufs seeds = { 0, 0, 0, 0, 0 };
  if (mgSeedsOfBatch (ms, 0, 0, (U32 *) b->dPacked, b->total, (U64 *) b->dOff, b->nReads, mgSeedGuess (ms->hasher->w, b->total), &seeds, &n, 0)) mgFatal ("query scan");
  U32 *six = (U32 *) malloc ((size_t) (n + 1) * 4), *spos = (U32 *) malloc ((size_t) (n + 1) * 4), *srid = (U32 *) malloc ((size_t) (n + 1) * 4);
  if (n && (mgMemcpyD2H (six, seeds.ix, n * 4, 0) || mgMemcpyD2H (spos, seeds.posF, n * 4, 0) || mgMemcpyD2H (srid, seeds.rid, n * 4, 0))) mgFatal ("D2H");
  mgSeedBufsFree (&seeds);
  for (U64 i = 0 ; i < n ; ++i) spos[i] &= MG_POS_MASK;

  U64 at = 0;
  for (int r = 0 ; r < nReads ; ++r)
    { U64 first = at;
      while (at < n && srid[at] == (U32) r) ++at;
      U32 ns = (U32) (at - first);
      const U32 *ix = six + first, *ps = spos + first;
      int missed = 0, copy[4] = { 0, 0, 0, 0 };
      for (U32 i = 0 ; i < ns ; ++i)
        if (ix[i]) ++copy[ms->info[ix[i]] & 3]; else ++missed;
      fprintf (out, "Q\t%s\t%llu\t%d miss, %d copy1, %d copy2, %d multi, %.2f hit\n",
               names[r], (unsigned long long) (offsets[r + 1] - offsets[r]), missed, copy[1], copy[2], copy[3],
               ((int) ns - missed) / (double) ((int) ns));
      /* chaining, modmap.c:213-276: occurrence number 0 doubles as "no block open"; a block is
         printed when it ends only with more than two copy-1 seeds, and the block left open at the
         end of the read only with more than two copy-2 seeds */
      U32 loc0 = 0, locN = 0, i0 = 0, iN = 0;
      int n1 = 0, n2 = 0;
      for (U32 i = 0 ; i < ns ; ++i)
        { U32 x = ix[i];
          if (!x || (ms->info[x] & 3) == 3) continue;
          U32 loc = ref->rev[ref->loc[x]];
          bool is1 = (ms->info[x] & 3) == 1;
          if (gVerbose)                                         /* modmap.c:218-229: printf, i.e. stdout whatever outFile is */
            { if (is1) printf ("  %6d\t%s %d\n", (int) ps[i], ref->names[ref->id[loc]], (int) ref->offset[loc]);
              else
                { U32 loc2 = ref->rev[ref->loc[x] + 1];
                  printf ("  %6d\t%s %d\t%s %d\n", (int) ps[i], ref->names[ref->id[loc]], (int) ref->offset[loc],
                          ref->names[ref->id[loc2]], (int) ref->offset[loc2]);
                }
            }
          bool end = blockEnds (ref, loc, loc0, locN, i0, iN, true);
          if (end && loc0 && !is1)
            { loc = ref->rev[ref->loc[x] + 1];
              end = blockEnds (ref, loc, loc0, locN, i0, iN, false);
            }
          if (end)
            { if (n1 > 2) printM (ref, out, names[r], ps, i0, iN, loc0, locN, n1, n2, copy[1]);
              n1 = n2 = 0; loc0 = loc; i0 = i;
            }
          if (is1) ++n1; else ++n2;
          locN = loc; iN = i;
        }
      if (n2 > 2) printM (ref, out, names[r], ps, i0, iN, loc0, locN, n1, n2, copy[1]);
    }
  free (six); free (spos); free (srid);
  return 0;
}

/* The batch is on the device already (2-bit packed, offsets in bases): mgQueryProcess uploads one, the file entry point
 * (mgQueryFile) gets its batches from the device text parser. */
int mgQueryProcessDevice (MgReference *ref, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, int nReads, const char **names, FILE *out)
{
  if (nReads <= 0) return 0;
  const int timing = mgKnobs ()->seedTiming == 1;          /* dev */
  struct timespec c0, c1; if (timing) clock_gettime (CLOCK_MONOTONIC, &c0);
  if (modsetSyncToHost (ref->ms, 0)) mgFatal ("modsetSyncToHost");
  int64_t *offsets = (int64_t *) malloc ((size_t) (nReads + 1) * 8);
  if (mgMemcpyD2H (offsets, dReadOffsets, (size_t) (nReads + 1) * 8, 0)) mgFatal ("D2H");
  MgDevBatch b; b.dPacked = (void *) dPacked; b.dOff = (void *) dReadOffsets; b.total = totalBases; b.nReads = (U32) nReads;
  MgChainQ *q = (MgChainQ *) malloc ((size_t) nReads * sizeof (MgChainQ));
  MgChainM *m = 0;                                         /* all reads' blocks, densely, in read order */
  const int hostChain = mgKnobs ()->queryHostChain == 1;   /* test knob */
  int rc = (hostChain || gVerbose) ? 1 : mgChainQueryDevice (ref, dPacked, totalBases, dReadOffsets, (U32) nReads, q, &m, MG_QUERY_MAXM, 0);
  if (rc < 0) mgFatal ("query");
  if (timing) clock_gettime (CLOCK_MONOTONIC, &c1);
  if (rc == 1) rc = queryProcessHostChain (ref, &b, offsets, nReads, names, out);
  else
    { double msF = 0, msW = 0;
      const int team = mgQueryLinesOut (ref, q, m, offsets, nReads, names, out, &msF, &msW);
      if (timing)
        fprintf (stderr, "mgQueryProcessDevice: %d reads: device (scan, lookups, chain, copies) %.1f ms, format %.1f ms (%d threads), write %.1f ms\n",
                 nReads, mgMsBetween (&c0, &c1), msF, team, msW);
    }
  free (q); free (m); free (offsets);
  return rc;
}
