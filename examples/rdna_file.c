/* examples/rdna_file.c — what `modasm -r stem -R ref.fa -T lo1 hi1 -T lo2 hi2 -rb 2 -w out` does (modasm.c:1574-1579,1602-1604), written against
 * include/modgpu.h in plain C: stem.mod + stem.readset are read back (mgReadsetLoad); the mods of the reference sequence and of the reads' rDNA
 * stretches are flagged (mgReadsetRefFlagFile: refFlag, modasm.c:752-860 -- the five counting lines); the flagged mods in a depth range are tested
 * against one another twice (mgReadsetTestMods: testMods, modasm.c:595-748 -- a "RUN" line each, and the files YY-TEST<n> and ZZ-TEST<n>, which this
 * program opens where it runs, as the reference does); the copy classes are reset to the non-repetitive core mods (mgReadsetResetBits: resetBits,
 * modasm.c:864-908) and out.mod + out.readset written.  The per-read and per-pair-of-mods work runs on the GPU; what depends on the order of the reads
 * is replayed on the host, so the lines are the reference's.  A -T that tests no mod ends the reference at its end; here it is an error before.
 *
 *   gcc -O2 -I include examples/rdna_file.c -o rdna_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./rdna_file stem ref.fa lo1 hi1 lo2 hi2 [out]
 */
#include <stdio.h>
#include <stdlib.h>
#include "modgpu.h"

static int testMods (MgReadset *rs, int lo, int hi)                                    /* -T lo hi */
{
  char yName[32], zName[32];
  const int run = mgReadsetTestModsRun (rs) + 1;
  sprintf (yName, "YY-TEST%d", run); sprintf (zName, "ZZ-TEST%d", run);
  FILE *y = fopen (yName, "w"), *z = fopen (zName, "w");
  const int rc = y && z ? mgReadsetTestMods (rs, lo, hi, y, z, stdout) : -1;
  if (y) fclose (y);
  if (z) fclose (z);
  return rc;
}

int main (int argc, char **argv)
{
  if (argc < 7) { fprintf (stderr, "usage: %s <stem of .mod + .readset> <ref.fa> <lo1> <hi1> <lo2> <hi2> [stem to write]\n", argv[0]); return 2; }
  MgReadset *rs = mgReadsetLoad (argv[1]);                                             /* -r stem */
  Modset *ms = rs->ms; Seqhash *sh = ms->hasher;
  U64 diag[4];
  if (mgReadsetRefFlagFile (rs, argv[2], stdout)) { fprintf (stderr, "FATAL ERROR: -R: %s\n", mgLastError ()); return 1; }      /* -R ref.fa */
  if (testMods (rs, atoi (argv[3]), atoi (argv[4])) || testMods (rs, atoi (argv[5]), atoi (argv[6]))) { fprintf (stderr, "FATAL ERROR: -T: %s\n", mgLastError ()); return 1; }
  const int path = mgReadsetRdnaPath (); mgReadsetRdnaDiag (diag);
  if (mgReadsetResetBits (rs, 2, stdout)) { fprintf (stderr, "FATAL ERROR: -rb: %s\n", mgLastError ()); return 1; }            /* -rb 2 */
  if (argc > 7) mgReadsetWrite (rs, argv[7]);                                          /* -w out */
  int nRdna = 0;
  const U8 *flags = mgReadsetReadFlags (rs);
  for (int i = 1 ; i <= rs->nReads ; ++i) nRdna += flags[i] & 1;
  fprintf (stderr, "rdna %s: the last -T took %llu batches for %llu tested mods, %llu visits, %llu partner occurrences; %d of %d reads are rDNA\n", path ? "by the host loops" : "on the device",
           (unsigned long long) diag[0], (unsigned long long) diag[1], (unsigned long long) diag[2], (unsigned long long) diag[3], nRdna, rs->nReads);
  mgReadsetDestroy (rs);
  modsetDestroy (ms); mgSeqhashDestroy (sh);                                           /* mgReadsetLoad made both (modasm.c:100-107) */
  return 0;
}
