/* examples/text_file.c — `modutils -rt in.txt [-p LO HI] -wt out.txt` (modutils.c:169-203) written against include/modgpu.h in plain
 * C: the text table is read on the GPU (mgModsetReadText: the file's lines parsed and the set built there), optionally pruned by depth
 * (modsetDepthPrune), and written back as text with the lines formatted on the GPU (mgModsetWriteTextDevice).  The summaries go to
 * stdout as the reference's do.
 *
 *   gcc -O2 -I include examples/text_file.c -o text_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./text_file -rt in.txt -p 2 40 -wt out.txt
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 5 || strcmp (argv[1], "-rt")) { fprintf (stderr, "usage: %s -rt in.txt [-p LO HI] -wt out.txt\n", argv[0]); return 2; }
  Modset *ms = mgModsetReadText (argv[2]);
  if (!ms) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
  modsetSummary (ms, stdout);
  for (int i = 3 ; i < argc ; )
    if (!strcmp (argv[i], "-p") && i + 2 < argc)
      { modsetDepthPrune (ms, atoi (argv[i + 1]), atoi (argv[i + 2])); modsetSummary (ms, stdout); i += 3; }
    else if (!strcmp (argv[i], "-wt") && i + 1 < argc)
      { FILE *f = fopen (argv[i + 1], "w");
        if (!f) { fprintf (stderr, "FATAL ERROR: failed to open text file %s\n", argv[i + 1]); return 1; }
        if (mgModsetWriteTextDevice (ms, f)) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
        fclose (f); i += 2;
      }
    else { fprintf (stderr, "FATAL ERROR: unknown command %s\n", argv[i]); return 1; }
  Seqhash *sh = ms->hasher;
  modsetDestroy (ms); mgSeqhashDestroy (sh);
  return 0;
}
