/* examples/paint_file.c — `modutils -c B k w s -a reads.fa [-a ...] -P ref.fa [-d depths.txt a.mod ...]` (modutils.c:33-51,65-77,
 * 260-273) written against include/modgpu.h in plain C: the set is built on the GPU from the read files (mgAddSequenceFile), every
 * record of ref.fa is painted with the depths of its modimizers (mgRefPaintFile: to stdout, as the reference's printf), and with -d
 * each entry's depth is reported beside its depth in the other sets (mgReportDepths), read as the reference's -r reads a .mod file.
 * As in the reference, -a comes first: N is base 0 only then (modutils.c:39).  The "added" lines go to stderr.
 *
 *   gcc -O2 -I include examples/paint_file.c -o paint_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./paint_file 20 21 64 17 -a reads.fa -P ref.fa -d depths.txt a.mod b.mod
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 7) { fprintf (stderr, "usage: %s B k w s -a reads.fa [...] [-P ref.fa] [-d depths.txt a.mod ...]\n", argv[0]); return 2; }
  Modset *ms = modsetCreate (seqhashCreate (atoi (argv[2]), atoi (argv[3]), atoi (argv[4])), atoi (argv[1]), 0);    /* -c */
  for (int i = 5 ; i + 1 < argc ; i += 2)
    if (!strcmp (argv[i], "-a") && mgAddSequenceFile (ms, argv[i + 1], stderr))
      { fprintf (stderr, "FATAL ERROR: failed to add %s: %s\n", argv[i + 1], mgLastError ()); return 1; }
    else if (!strcmp (argv[i], "-P") && mgRefPaintFile (ms, argv[i + 1], stdout))
      { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
    else if (!strcmp (argv[i], "-d"))
      { FILE *fd = fopen (argv[i + 1], "w");
        int n = argc - i - 2;
        Modset **others = (Modset **) malloc ((size_t) (n > 0 ? n : 1) * sizeof (Modset *));
        if (!fd || !others) { fprintf (stderr, "FATAL ERROR: failed to open depths file %s\n", argv[i + 1]); return 1; }
        for (int j = 0 ; j < n ; ++j)
          { FILE *f = mgFzOpen (argv[i + 2 + j], "r");
            if (!f) { fprintf (stderr, "FATAL ERROR: failed to open mod file %s\n", argv[i + 2 + j]); return 1; }
            others[j] = modsetRead (f); fclose (f);
          }
        if (mgReportDepths (ms, others, n, fd)) { fprintf (stderr, "FATAL ERROR: %s\n", mgLastError ()); return 1; }
        fclose (fd);
        for (int j = 0 ; j < n ; ++j) modsetDestroy (others[j]);
        free (others);
        break;                                                         /* -d takes the rest of the line */
      }
  modsetDestroy (ms);
  return 0;
}
