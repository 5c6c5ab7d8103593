/* examples/gunzip_file.c — `gzip -dc in.gz > out`, written against include/modgpu.h in plain C: an ordinary gzip file (one member or several, no
 * block table) crosses to the device compressed and is inflated there chunk by chunk (mgGzipInflateFile); the text comes back and is written
 * behind the call by a writer thread.  "-" as out is stdout.
 *
 *   gcc -O2 -I include examples/gunzip_file.c -o gunzip_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./gunzip_file in.gz out [anything: a line about the call to stderr]
 */
#include <stdio.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 3) { fprintf (stderr, "usage: %s <in.gz> <out | ->\n", argv[0]); return 2; }
  const int rc = mgGzipInflateFile (argv[1], argv[2], stderr);
  if (rc == -2) { fprintf (stderr, "%s is not an ordinary gzip file (a BGZF file is mgBgzfInflateFile's)\n", argv[1]); return 3; }
  if (rc) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  U64 d[8];
  mgGunzipDiag (d);
  if (argc > 3) fprintf (stderr, "%llu members in %llu batches: %llu chunks confirmed, %llu discarded, %llu folded, %llu capacity retries\n", (unsigned long long) d[5],
                         (unsigned long long) d[4], (unsigned long long) d[1], (unsigned long long) d[2], (unsigned long long) d[3], (unsigned long long) d[6]);
  return 0;
}
