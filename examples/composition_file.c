/* examples/composition_file.c — what `composition -b -q -l reads.fq` does (composition.c:32-121), written against include/modgpu.h in
 * plain C: the file's records, lengths, bases and qualities, counted on the device (mgCompositionFile).  The program's lines go to
 * stdout, "incomplete sequence record line N" -- a last record that is cut off is dropped, as the reference drops it -- to stderr.
 * FASTA or FASTQ, plain or gzip'd.
 *
 *   gcc -O2 -I include examples/composition_file.c -o composition_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./composition_file reads.fq [anything: a line about the call to stderr]
 */
#include <stdio.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 2) { fprintf (stderr, "usage: %s <reads.fa | reads.fq>[.gz]\n", argv[0]); return 2; }
  MgComposition res;
  if (mgCompositionFile (argv[1], MG_COMP_BASES | MG_COMP_QUALS | MG_COMP_LENGTHS, stdout, stderr, &res))
    { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  U64 diag[4];
  mgCompositionDiag (diag);
  if (argc > 2) fprintf (stderr, "%llu records in %u length bins; %llu windows, %llu tiles, %llu kernels\n", (unsigned long long) res.nSeq, res.nBins,
                         (unsigned long long) diag[0], (unsigned long long) diag[1], (unsigned long long) diag[3]);
  mgCompositionFree (&res);
  return 0;
}
