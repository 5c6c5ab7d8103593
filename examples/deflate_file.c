/* examples/deflate_file.c — `bgzip -c in > out.gz` and `seqconvert -fa|-fq|-hoco -o out.fa.gz in`, written against include/modgpu.h in plain C:
 * the text is deflated ON THE DEVICE into BGZF members of 65280 text bytes, one workgroup a block (mgBgzfDeflateFile, mgSeqConvertFileBgzf);
 * only the compressed file comes back and is written behind the call by a writer thread.  What it writes, bgzip -d, samtools, tabix and
 * this library's own device reader (examples/inflate_file.c, mgCompositionFile, mgSeqConvertFile) read block-parallel.
 *
 *   gcc -O2 -I include examples/deflate_file.c -o deflate_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./deflate_file in out.gz                   bgzip
 *   ./deflate_file -fa|-fq|-hoco in out.gz     seqconvert / seqhoco, the output as BGZF
 */
#include <stdio.h>
#include <string.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  int flags = -1, rc;
  MgSeqConvert res;
  U64 diag[4];
  if (argc == 4) flags = !strcmp (argv[1], "-fa") ? MG_SEQ_FASTA : !strcmp (argv[1], "-fq") ? MG_SEQ_FASTQ : !strcmp (argv[1], "-hoco") ? MG_SEQ_HOCO : -1;
  if (argc != 3 && !(argc == 4 && flags >= 0)) { fprintf (stderr, "usage: %s [-fa | -fq | -hoco] <in> <out.gz | ->\n", argv[0]); return 2; }
  rc = argc == 3 ? mgBgzfDeflateFile (argv[1], argv[2], stderr) : mgSeqConvertFileBgzf (argv[2], argv[3], flags, stderr, &res);
  if (rc) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  mgDeflateDiag (diag);
  if (argc == 4) fprintf (stderr, "written %llu sequences, total length %llu\n", (unsigned long long) res.nSeq, (unsigned long long) res.totSeqLen);
  fprintf (stderr, "%llu blocks deflated on the device in %llu launches: %llu bytes of text, %llu bytes of members\n",
           (unsigned long long) diag[0], (unsigned long long) diag[3], (unsigned long long) diag[1], (unsigned long long) diag[2]);
  return 0;
}
