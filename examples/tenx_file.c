/* examples/tenx_file.c — `modutils -c B k w s -x reads.fq -s a b c -sM m -H his -wt out` (modutils.c:139-157,205-228,240-244,191-199)
 * written against include/modgpu.h in plain C.  The 10x reads are parsed, trimmed and added on the GPU (mgAddSequenceFile10x), the copy
 * classes are set where the depths are (mgModsetSetCopy / mgModsetSetCopyM) and every summary is counted there (mgModsetSummaryDevice):
 * the set's value[] and depth[] never come to the host.  stdout is the reference's, without its timing lines.
 *
 *   gcc -O2 -I include examples/tenx_file.c -o tenx_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./tenx_file -c 20 11 4 17 -x reads.fq -s 2 3 6 -sM 5 -H his.txt -wt out.txt
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"

static void fatal (const char *what) { fprintf (stderr, "FATAL ERROR: %s\n", what); exit (1); }

int main (int argc, char **argv)
{
  if (argc < 6 || strcmp (argv[1], "-c")) { fprintf (stderr, "usage: %s -c B k w s [-x reads] [-s a b c] [-sM m] [-H his] [-wt out]\n", argv[0]); return 2; }
  Seqhash *sh = seqhashCreate (atoi (argv[3]), atoi (argv[4]), atoi (argv[5]));
  seqhashReport (sh, stdout);
  Modset *ms = modsetCreate (sh, atoi (argv[2]), 0);
  for (int i = 6 ; i < argc ; )
    { int rc = 0, summary = 1;
      FILE *f = 0;
      if (!strcmp (argv[i], "-x") && i + 1 < argc) { rc = mgAddSequenceFile10x (ms, argv[i + 1], stdout); i += 2; }
      else if (!strcmp (argv[i], "-s") && i + 3 < argc) { rc = mgModsetSetCopy (ms, atoi (argv[i + 1]), atoi (argv[i + 2]), atoi (argv[i + 3])); i += 4; }
      else if (!strcmp (argv[i], "-sM") && i + 1 < argc) { rc = mgModsetSetCopyM (ms, atoi (argv[i + 1])); i += 2; }
      else if ((!strcmp (argv[i], "-H") || !strcmp (argv[i], "-wt")) && i + 1 < argc)
        { if (!(f = fopen (argv[i + 1], "w"))) fatal ("failed to open an output file");
          if (argv[i][1] == 'H') mgDepthHistogram (ms, f); else rc = mgModsetWriteTextDevice (ms, f);
          fclose (f); summary = 0; i += 2;
        }
      else fatal ("unknown command");
      if (rc || (summary && mgModsetSummaryDevice (ms, stdout))) fatal (mgLastError ());
    }
  modsetDestroy (ms); mgSeqhashDestroy (sh);
  return 0;
}
