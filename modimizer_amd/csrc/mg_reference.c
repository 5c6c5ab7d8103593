/* mg_reference.c — modmap's Reference (modmap.c:49-134): made, fed batch by batch, classified and packed.
 * A batch is on the device already; its scan, inserts and occurrences stay there (mg_reads.hip, mg_refpack.hip).  What remains on the
 * host is the reference's own serial bookkeeping -- names, lengths, the report lines -- restated with its quirks because its printed
 * output is the parity target.
 */
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"
#include "mg_internal.h"

MgReference *mgReferenceCreate (Modset *ms, U32 size)
{
  if (!ms || !ms->size) { fprintf (stderr, "FATAL ERROR: modset must be initialised before reference\n"); exit (-1); }
  if (!size) { fprintf (stderr, "FATAL ERROR: refCreate must have size > 0\n"); exit (-1); }
  MgReference *ref = (MgReference *) calloc (1, sizeof (MgReference));
  ref->ms = ms;
  ref->size = size;
  ref->depth = (U32 *) calloc (ms->size, sizeof (U32));
  ref->index = (U32 *) malloc ((size_t) size * sizeof (U32));
  ref->offset = (U32 *) malloc ((size_t) size * sizeof (U32));
  ref->id = (U32 *) malloc ((size_t) size * sizeof (U32));
  return ref;
}

void mgReferenceDestroy (MgReference *ref)
{
  if (!ref) return;
  mgChainForget (ref);
  free (ref->depth); free (ref->loc); free (ref->rev);
  free (ref->index); free (ref->offset); free (ref->id);
  for (int i = 0 ; i < ref->nSeq ; ++i) free (ref->names[i]);
  free (ref->names); free (ref->len); free (ref);
}

/* the names and lengths of nSeq more sequences; the reference die()s on a duplicate name (modmap.c:102) */
static void refRegister (MgReference *ref, const char **names, const int64_t *offsets, int nSeq)
{
  ref->names = (char **) realloc (ref->names, (size_t) (ref->nSeq + nSeq) * sizeof (char *));
  ref->len = (U32 *) realloc (ref->len, (size_t) (ref->nSeq + nSeq) * sizeof (U32));
  /* an open-addressed set of the names seen so far (the reference keeps them in a DICT): a fragmented assembly
     has 1e5 - 1e6 contigs, so no pairwise comparison */
  const size_t all = (size_t) ref->nSeq + (size_t) nSeq;
  size_t cap = 16; while (cap < 4 * all) cap *= 2;
  int *slot = (int *) calloc (cap, sizeof (int));                       /* 1 + position in ref->names; 0 = empty */
  for (size_t i = 0 ; i < all ; ++i)
    { const char *nm = i < (size_t) ref->nSeq ? ref->names[i] : names[i - ref->nSeq];
      U64 h = 0xcbf29ce484222325ull;
      for (const unsigned char *c = (const unsigned char *) nm ; *c ; ++c) h = (h ^ *c) * 0x100000001b3ull;
      size_t at = (size_t) (h ^ (h >> 29)) & (cap - 1);
      while (slot[at])
        { if (!strcmp (ref->names[slot[at] - 1], nm))
            { fprintf (stderr, "FATAL ERROR: duplicate ref sequence name %s\n", nm); exit (-1); }
          at = (at + 1) & (cap - 1);
        }
      slot[at] = (int) i + 1;
      if (i >= (size_t) ref->nSeq)
        { ref->names[i] = strdup (nm);
          ref->len[i] = (U32) (offsets[i - ref->nSeq + 1] - offsets[i - ref->nSeq]);
        }
    }
  free (slot);
}

/* modmap.c:106-118 for a batch of sequences that is on the device already (2-bit packed, offsets in bases): scan + insert
 * (or lookup) there, the (index, offset, id) of every occurrence appended here */
int mgReferenceAddDevice (MgReference *ref, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, int nSeq, const char **names, bool isAdd)
{
  Modset *ms = ref->ms;
  int64_t *offsets = (int64_t *) malloc ((size_t) (nSeq + 1) * 8);
  if (mgMemcpyD2H (offsets, dReadOffsets, (size_t) (nSeq + 1) * 8, 0)) mgFatal ("D2H");
  refRegister (ref, names, offsets, nSeq);
  free (offsets);
  U64 n = 0;
  MgSeedBufs seeds = { 0, 0, 0, 0, 0 };
  const int timing = mgKnobs ()->seedTiming == 1;          /* dev */
  struct timespec a0, a1, a2, a3; clock_gettime (CLOCK_MONOTONIC, &a0);
  const MgStatus s = mgSeedsOfBatch (ms, 0, isAdd, dPacked, totalBases, dReadOffsets, (U32) nSeq, mgSeedGuess (ms->hasher->w, totalBases), &seeds, &n, 0);
  if (s == MG_ERR_CAPACITY) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); exit (-1); }   /* modset.c:58 */
  if (s) mgFatal ("reference scan");
  clock_gettime (CLOCK_MONOTONIC, &a1);
  /* modmap.c:110-117: the occurrences stay on the device (mg_refpack.hip), appended in order behind those of earlier batches */
  U32 added = 0;
  MgStatus as = mgRefBuildAppend (ref, seeds.ix, seeds.posF, seeds.rid, n, (U32) ref->nSeq, &added);
  if (as == MG_ERR_CAPACITY) { fprintf (stderr, "FATAL ERROR: reference size overflow\n"); exit (-1); }      /* modmap.c:111 */
  if (as) mgFatal ("reference append");
  ref->max += added;
  clock_gettime (CLOCK_MONOTONIC, &a2);
  mgSeedBufsFree (&seeds);
  clock_gettime (CLOCK_MONOTONIC, &a3);
  if (timing) fprintf (stderr, "mgReferenceAddDevice: %.3f Gbp, %d sequences: allocations + scan + insert %.1f ms, append %.1f ms, frees %.1f ms\n", totalBases / 1e9, nSeq,
                       mgMsBetween (&a0, &a1), mgMsBetween (&a1, &a2), mgMsBetween (&a2, &a3));
  ref->nSeq += nSeq;
  return 0;
}

/* modmap.c:120-133: the report of a file, the copy classes, the packed arrays.  Classification, loc (exclusive sums) and rev (stable
   sort of the occurrences by index) are made on the device from the occurrences it holds (mg_refpack.hip); the host's arrays -- sized
   as referencePack sizes them (modmap.c:76-81) -- receive them in one piece each */
void mgReferenceFinish (MgReference *ref, U64 totLen, bool isAdd, FILE *out)
{
  Modset *ms = ref->ms;
  fprintf (out, "  %d hashes from %d reference sequences, total length %lld\n", ref->max, ref->nSeq, (long long) totLen);
  const int timing = mgKnobs ()->seedTiming == 1;          /* dev */
  struct timespec f0, f1, f2, f3; clock_gettime (CLOCK_MONOTONIC, &f0);
  { U32 again[3];
    if (mgRefPackedTallies (ref, again))                  /* a further file that added nothing to a packed Reference (one that adds died in the append, modmap.c:111): */
      { fprintf (out, "  %d copy 1, %d copy 2, %d multiple\n", again[0], again[1], again[2]);      /* the classes and the packed arrays are what they were */
        if (isAdd) modsetPack (ms);
        return;
      }
  }
  if (modsetSyncToHost (ms, 0)) mgFatal ("modsetSyncToHost");       /* value[] of the new entries */
  clock_gettime (CLOCK_MONOTONIC, &f1);
  const U32 n = ref->max ? ref->max : 1, m = ms->max + 1;
  free (ref->index); free (ref->offset); free (ref->id); free (ref->depth); free (ref->rev); free (ref->loc);   /* (nothing was written into them: the occurrences are on the device) */
  ref->index = (U32 *) mgAllocBig ((size_t) n * sizeof (U32));
  ref->offset = (U32 *) mgAllocBig ((size_t) n * sizeof (U32));
  ref->id = (U32 *) mgAllocBig ((size_t) n * sizeof (U32));
  ref->rev = (U32 *) mgAllocBig ((size_t) n * sizeof (U32));
  ref->depth = (U32 *) mgAllocBig ((size_t) (m > ms->size ? m : ms->size) * sizeof (U32));
  ref->loc = (U32 *) mgAllocBig ((size_t) m * sizeof (U32));
  if (!ref->index || !ref->offset || !ref->id || !ref->rev || !ref->depth || !ref->loc) { fprintf (stderr, "FATAL ERROR: out of memory\n"); exit (-1); }
  ref->size = ref->max;
  U32 tal[3];
  clock_gettime (CLOCK_MONOTONIC, &f2);
  if (mgRefBuildFinish (ref, ref->index, ref->offset, ref->id, ref->depth, ref->rev, ref->loc, ms->info, tal)) mgFatal ("reference pack");
  clock_gettime (CLOCK_MONOTONIC, &f3);
  if (timing) fprintf (stderr, "mgReferenceFinish: modset mirror %.1f ms, host arrays %.1f ms, classes + loc + rev + mirror %.1f ms\n",
                       mgMsBetween (&f0, &f1), mgMsBetween (&f1, &f2), mgMsBetween (&f2, &f3));
  if ((size_t) ms->size > (size_t) m) memset (ref->depth + m, 0, ((size_t) ms->size - m) * sizeof (U32));      /* (the reference's resize keeps ms->size zeroed entries when the set is not packed) */
  fprintf (out, "  %d copy 1, %d copy 2, %d multiple\n", tal[0], tal[1], tal[2]);
  if (isAdd) modsetPack (ms);
}
