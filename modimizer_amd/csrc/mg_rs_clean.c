/* mg_rs_clean.c — modasm -C and -P over a read set (cleanMods, modasm.c:514-555; readProperties, modasm.c:912-952).
 * Both ask how often one read holds one mod; the reference clears an array of ms->max + 1 entries per read to find out.  On the device
 * (mg_rsdev.hip) the hits are sorted by mod; the host loops below, for a set of 2^32 - 16 hits or more, a device without room or
 * MODGPU_READSET_HOST=1, stamp the array with the read's number instead of clearing it.  Same bytes either way. */
#include "mg_readset_int.h"

static __thread int gCleanPath = -1, gPropertiesPath = -1;
int mgReadsetCleanModsPath (void) { return gCleanPath; }
int mgReadsetPropertiesPath (void) { return gPropertiesPath; }

static void cleanModsHost (MgReadset *rs, U32 counts[3])
{
  Modset *ms = rs->ms;
  const int w = ms->hasher->w;
  U32 *inRead = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32));      /* the last read (from 1) that held the mod */
  for (int r = 1 ; r < rs->nReads ; ++r)                                   /* modasm.c:522-523: the last read is never looked at */
    { const U64 a = rs->hitStart[r], e = rs->hitStart[r + 1];
      for (U64 h = a ; h < e ; ++h)
        { const U32 hh = rs->hit[h] & TOPMASK;
          if (inRead[hh] == (U32) r) msSetRepeat (ms, hh);
          inRead[hh] = (U32) r;
          if (h == a) continue;
          if ((int) rs->dx[h] < w && h + 1 < e && (int) rs->dx[h + 1] < w) msSetInternal (ms, hh);
          const U32 hhLast = rs->hit[h - 1] & TOPMASK;
          const int lastDepth = ms->depth[hhLast], thisDepth = ms->depth[hh];
          if (lastDepth > 2 * thisDepth) msSetMinor (ms, hh);
          if (thisDepth > 2 * lastDepth) msSetMinor (ms, hhLast);
        }
    }
  free (inRead);
  counts[0] = counts[1] = counts[2] = 0;
  for (U64 i = 0 ; i <= ms->max ; ++i)
    { if (msIsRepeat (ms, i)) ++counts[0];
      if (msIsInternal (ms, i)) ++counts[1];
      if (msIsMinor (ms, i)) ++counts[2];
    }
  mgRsCopyTallies (rs, ms->info, 1, (int *) rs->nCopy);                     /* invBuild's nCopy[] (modasm.c:273-277) */
}

int mgReadsetCleanMods (MgReadset *rs, FILE *out)                 /* modasm.c:514-555 */
{
  gCleanPath = -1;
  Modset *ms = rs->ms;
  if (modsetSyncToHost (ms, 0)) return -1;
  U32 counts[3] = { 0, 0, 0 };
  int host = rsHostForced (rs);
  if (!host)
    { MgRsView v; mgRsViewOf (rs, &v);
      const int rc = mgReadsetCleanDevice (&v, ms->info, (int *) rs->nCopy, counts);
      if (rc < 0) return -1;
      host = rc;
    }
  if (host) cleanModsHost (rs, counts);
  gCleanPath = host;
  /* invBuild (modasm.c:552): the lists are a function of the hits and of depth[]; they are made again only if depth[] no longer gives the places held */
  if (!rs->invStart || !rs->invSpace || mgRsInvPlaces (ms, 0, rs->invStart) == ~(U64) 0) mgRsInvBuildHost (rs, 0);
  mgModsetHostChanged (ms);                                        /* info[] is new: a device table is made again from the host arrays on its next use */
  fprintf (out, "set %d repeated, %d internal, %d minor_variant mods\n", (int) counts[0], (int) counts[1], (int) counts[2]);
  return 0;
}

typedef struct { U32 *ev; U32 n, cap; } RsEvents;      /* triples (read, mod | TOPBIT if in one orientation, count) */

static void propertiesHost (MgReadset *rs, int *tally, RsEvents *E)
{
  Modset *ms = rs->ms;
  U32 *f = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32)), *r = (U32 *) calloc ((size_t) ms->max + 1, sizeof (U32));
  U32 *seen = 0; U64 capSeen = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { const U64 a = rs->hitStart[i], e = rs->hitStart[i + 1];
      if (e - a > capSeen) { capSeen = e - a; seen = (U32 *) realloc (seen, capSeen * sizeof (U32)); }
      U64 nSeen = 0;
      for (U64 j = a ; j < e ; ++j)
        { const U32 h = rs->hit[j] & TOPMASK;
          if (!msIsCopy1 (ms, h)) continue;
          if (!f[h] && !r[h]) seen[nSeen++] = h;
          if (rs->hit[j] & TOPBIT) ++f[h]; else ++r[h];
        }
      qsort (seen, nSeen, sizeof (U32), rsU32Cmp);                  /* distinct mods: any sort gives the one ascending order */
      int *t = tally + 5 * (size_t) i;
      for (U64 q = 0 ; q < nSeen ; ++q)
        { const U32 h = seen[q], nf = f[h], nr = r[h];
          f[h] = r[h] = 0;
          ++t[0];
          if (nf + nr == 1) continue;
          if (nf == 1 && nr == 1) ++t[2];
          else if (nf + nr == 2) ++t[1];
          else
            { const int tan = !nf || !nr;
              ++t[tan ? 3 : 4];
              if (E->n == E->cap) { E->cap = E->cap ? E->cap * 2 : 1024; E->ev = (U32 *) realloc (E->ev, (size_t) E->cap * 12); }
              U32 *v = E->ev + 3 * (size_t) E->n++;
              v[0] = (U32) i; v[1] = h | (tan ? TOPBIT : 0); v[2] = nf + nr;
            }
        }
    }
  free (f); free (r); free (seen);
}

int mgReadsetProperties (MgReadset *rs, FILE *out)                /* modasm.c:912-952 */
{
  gPropertiesPath = -1;
  Modset *ms = rs->ms;
  if (modsetSyncToHost (ms, 0)) return -1;
  int *tally = (int *) calloc (((size_t) rs->nReads + 1) * 5, sizeof (int));      /* per read { n, n2Tan, n2Rev, nMoreTan, nMoreRev } */
  RsEvents E = { 0, 0, 0 };
  int host = rsHostForced (rs);
  if (!host)
    { MgRsView v; mgRsViewOf (rs, &v);
      const int rc = mgReadsetPropertiesDevice (&v, tally, &E.ev, &E.n);
      if (rc < 0) { free (tally); return -1; }
      host = rc;
    }
  if (host) propertiesHost (rs, tally, &E);
  gPropertiesPath = host;
  /* the lines (one short one per read, and one per mod that a read holds more than twice in one orientation): the events are in (read, mod) order */
  U32 e = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i)
    { const int *t = tally + 5 * (size_t) i;
      const U32 e0 = e;
      for ( ; e < E.n && E.ev[3 * (size_t) e] == (U32) i ; ++e)
        if (E.ev[3 * (size_t) e + 1] & TOPBIT) fprintf (out, "MT i %d h %d count %d\n", i, (int) (E.ev[3 * (size_t) e + 1] & TOPMASK), (int) E.ev[3 * (size_t) e + 2]);
      fprintf (out, "READ %d n %d n2Tan %d n2Rev %d nMoreTan %d nMoreRev %d\n", i, t[0], t[1], t[2], t[3], t[4]);
      if (t[3] > 5)
        { fprintf (out, "RM %d nMoreTan %d", i, t[3]);
          for (U32 j = e0 ; j < e ; ++j) fprintf (out, " %d", (int) (E.ev[3 * (size_t) j + 1] & TOPMASK));
          fputc ('\n', out);
        }
    }
  free (tally); free (E.ev);
  return 0;
}
