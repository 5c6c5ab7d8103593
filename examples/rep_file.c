/* examples/rep_file.c — what `modrep -R ref.fa ref.mod -s3 reads.fa reads.mod` does (modrep.c:582-583,594-596), written against
 * include/modgpu.h in plain C: the one reference sequence is located in its set (mgRepRefCreate: refCreate, modrep.c:27-63 -- its line
 * "found .. of .. locations in ref length .."), every read is voted onto the reference's strand from its first 100 reference hits, the bad
 * ones reported, the others oriented, scanned again and their mods of the second set tallied (mgRepAnalyze3File: analyzeSequences3,
 * modrep.c:170-268 -- the BADREAD lines on stdout, "read .. reads, .." and "minimum max for a read is .." on stderr).  Scans, lookups, the
 * votes, the reverse complements and the tallies run on the GPU.  The .mod files may be gzip'd or plain.
 *
 *   gcc -O2 -I include examples/rep_file.c -o rep_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./rep_file ref.fa ref.mod reads.fa reads.mod
 */
#include <stdio.h>
#include <stdlib.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 5) { fprintf (stderr, "usage: %s <ref.fa> <ref.mod> <reads.fa> <reads.mod>\n", argv[0]); return 2; }
  MgRepRef *ref = mgRepRefCreate (argv[1], argv[2], stderr);                           /* -R ref.fa ref.mod */
  if (!ref) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  MgRepResult res;
  if (mgRepAnalyze3File (ref, argv[3], argv[4], stdout, stderr, &res))                 /* -s3 reads.fa reads.mod */
    { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  int flipped = 0;
  for (int i = 0 ; i < res.nRead ; ++i) if (!res.bad[i] && !res.isF[i]) ++flipped;
  if (argc > 5) fprintf (stderr, "%d of %d good reads reverse-complemented, %llu hits, %s\n", flipped, res.nGood,
                         (unsigned long long) res.hitStart[res.nGood], mgRepPath () ? "not on the device" : "on the device");
  mgRepResultFree (&res);
  mgRepRefDestroy (ref);
  return 0;
}
