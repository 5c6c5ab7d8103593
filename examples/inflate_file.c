/* examples/inflate_file.c — `bgzip -d -c in.gz > out`, written against include/modgpu.h in plain C: a blocked-gzip (BGZF) file's members
 * cross to the device compressed and are inflated there, one wave a member (mgBgzfInflateFile); the text comes back and is written behind
 * the call by a writer thread.  "-" as out is stdout.
 *
 *   gcc -O2 -I include examples/inflate_file.c -o inflate_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./inflate_file in.gz out [anything: a line about the call to stderr]
 */
#include <stdio.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 3) { fprintf (stderr, "usage: %s <in.gz> <out | ->\n", argv[0]); return 2; }
  const int rc = mgBgzfInflateFile (argv[1], argv[2], stderr);
  if (rc == -2) { fprintf (stderr, "%s is not a BGZF file from end to end (an ordinary gzip file is zlib's business)\n", argv[1]); return 3; }
  if (rc) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  U64 diag[4];
  mgInflateDiag (diag);
  if (argc > 3) fprintf (stderr, "%llu members inflated on the device in %llu launches: %llu compressed bytes up, %llu bytes of text\n",
                         (unsigned long long) diag[0], (unsigned long long) diag[3], (unsigned long long) diag[1], (unsigned long long) diag[2]);
  return 0;
}
