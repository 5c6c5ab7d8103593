/* examples/rep1_file.c — what `modrep -R ref.fa ref.mod -s1 reads.fa reads.mod -s2 reads.fa reads.mod` does (modrep.c:582-593), written
 * against include/modgpu.h in plain C.  -s1 (mgRepAnalyze1File: analyzeSequences1, modrep.c:272-489) orients the reads as -s3 does, then
 * prunes mods and reads on the device -- five "NMOD" lines, then "MOD", "BLOCK" and "READ" on stdout, "read .. reads, .." and
 * "reduced .. reads to .. reads" on stderr.  -s2 (mgRepAnalyze2File: analyzeSequences2, modrep.c:498-539) counts the reads that hold
 * two neighbouring ones of four reference entries: "n1 .. n2 .. n3 .. n4 ..".  The .mod files may be gzip'd or plain.
 *
 *   gcc -O2 -I include examples/rep1_file.c -o rep1_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./rep1_file ref.fa ref.mod reads.fa reads.mod
 */
#include <stdio.h>
#include <stdlib.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 5) { fprintf (stderr, "usage: %s <ref.fa> <ref.mod> <reads.fa> <reads.mod>\n", argv[0]); return 2; }
  MgRepRef *ref = mgRepRefCreate (argv[1], argv[2], stderr);                           /* -R ref.fa ref.mod */
  if (!ref) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  MgRep1Result res;
  if (mgRepAnalyze1File (ref, argv[3], argv[4], stdout, stderr, &res))                 /* -s1 reads.fa reads.mod */
    { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  U64 diag[8];
  mgRep1Diag (diag);
  if (argc > 5) fprintf (stderr, "%d of %d good reads kept, %llu links in the largest of %llu builds, %llu kernels\n", res.readsAfter, res.nGood,
                         (unsigned long long) diag[1], (unsigned long long) diag[0], (unsigned long long) diag[6]);
  mgRep1ResultFree (&res);
  int counts[4];
  if (mgRepAnalyze2File (ref, argv[3], argv[4], stdout, counts))                       /* -s2 reads.fa reads.mod */
    { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  mgRepRefDestroy (ref);
  return 0;
}
