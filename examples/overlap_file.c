/* examples/overlap_file.c — what `modasm -r stem -b -c -o2 d -w out` does (modasm.c:1574-1579,1586-1596), written against include/modgpu.h in
 * plain C: stem.mod + stem.readset are read back (mgReadsetLoad), the bad reads are marked from every read's overlaps (mgReadsetMarkBadReads:
 * markBadReads, modasm.c:1266-1322 -- the three "MB" lines), then the contained ones among the rest (mgReadsetMarkContained: markContained,
 * modasm.c:1370-1394 -- the "MC" line), the overlap statistics of every d'th read are printed as they stand with those flags set
 * (mgReadsetOverlapStats: the "RR" lines of findOverlaps, modasm.c:314-418) and out.mod + out.readset written with the flags in them.  What a
 * pair of reads shares is worked out on the GPU, a batch of query reads at a time; what depends on the order of the commands is replayed on
 * the host, so the lines are the reference's.
 *
 *   gcc -O2 -I include examples/overlap_file.c -o overlap_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./overlap_file stem d [out]
 */
#include <stdio.h>
#include <stdlib.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 3 || atoi (argv[2]) < 1) { fprintf (stderr, "usage: %s <stem of .mod + .readset> <d: every d'th read> [stem to write]\n", argv[0]); return 2; }
  MgReadset *rs = mgReadsetLoad (argv[1]);                                             /* -r stem */
  Modset *ms = rs->ms; Seqhash *sh = ms->hasher;
  U64 diag[4];
  if (mgReadsetMarkBadReads (rs, stdout)) { fprintf (stderr, "FATAL ERROR: -b: %s\n", mgLastError ()); return 1; }      /* -b */
  const int pathB = mgReadsetOverlapsPath (); mgReadsetOverlapsDiag (diag);
  if (mgReadsetMarkContained (rs, stdout)) { fprintf (stderr, "FATAL ERROR: -c: %s\n", mgLastError ()); return 1; }    /* -c */
  if (mgReadsetOverlapStats (rs, (U32) atoi (argv[2]), stdout)) { fprintf (stderr, "FATAL ERROR: -o2: %s\n", mgLastError ()); return 1; }      /* -o2 d */
  if (argc > 3) mgReadsetWrite (rs, argv[3]);                                          /* -w out */
  int nBad = 0, nContained = 0;
  for (int i = 1 ; i <= rs->nReads ; ++i) { nBad += rs->bad[i] != 0; nContained += rs->contained[i] != 0; }
  fprintf (stderr, "overlaps %s: -b took %llu batches, %llu candidates, %llu pairs; %d of %d reads bad, %d contained\n", pathB ? "by the host loops" : "on the device",
           (unsigned long long) diag[0], (unsigned long long) diag[1], (unsigned long long) diag[2], nBad, rs->nReads, nContained);
  mgReadsetDestroy (rs);
  modsetDestroy (ms); mgSeqhashDestroy (sh);                                           /* mgReadsetLoad made both (modasm.c:100-107) */
  return 0;
}
