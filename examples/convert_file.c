/* examples/convert_file.c — what `seqconvert -fa|-fq -S -o out in` (seqconvert.c) and `seqhoco in > out` (seqhoco.c) do, written against
 * include/modgpu.h in plain C: a FASTA or FASTQ file, plain or gzip'd, rewritten on the device (mgSeqConvertFile).  "incomplete sequence
 * record line N" -- a last record that is cut off is dropped, as the reference drops it -- goes to stderr.  An out name that ends in .gz
 * is written as gzip; "-" is stdout.
 *
 *   gcc -O2 -I include examples/convert_file.c -o convert_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./convert_file -fa|-fq|-hoco out in [anything: a line about the call to stderr]
 */
#include <stdio.h>
#include <string.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  const int flags = argc < 4 ? 0 : !strcmp (argv[1], "-fa") ? MG_SEQ_FASTA : !strcmp (argv[1], "-fq") ? MG_SEQ_FASTQ : !strcmp (argv[1], "-hoco") ? MG_SEQ_HOCO : 0;
  if (!flags) { fprintf (stderr, "usage: %s -fa|-fq|-hoco <out.fa | out.fq>[.gz] <reads.fa | reads.fq>[.gz]\n", argv[0]); return 2; }
  MgSeqConvert res;
  if (mgSeqConvertFile (argv[3], argv[2], flags, stderr, &res))
    { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  U64 diag[4];
  mgSeqConvertDiag (diag);
  if (argc > 4) fprintf (stderr, "written %llu sequences to file type %s, total length %llu, max length %llu; %llu windows, %llu tiles, %llu kernels\n",
                         (unsigned long long) res.nSeq, res.outType == 2 ? "fastq" : "fasta", (unsigned long long) res.totSeqLen, (unsigned long long) res.maxSeqLen,
                         (unsigned long long) diag[0], (unsigned long long) diag[1], (unsigned long long) diag[3]);
  return 0;
}
