/* examples/clean_file.c — what `modasm -r stem -C -P -w out` does (modasm.c:1574-1579,1601,1605), written against include/modgpu.h in plain C:
 * stem.mod + stem.readset are read back (mgReadsetLoad: readsetRead, modasm.c:128-149), the repeat / internal / minor-variant flags of the
 * mods are set from the reads' hit lists (mgReadsetCleanMods: cleanMods, modasm.c:514-555 -- its line "set .. repeated, .. internal, ..
 * minor_variant mods"; like the reference it never looks at the LAST read), every read's copy-1 mods are classified (mgReadsetProperties:
 * readProperties, modasm.c:912-952 -- the MT / READ / RM lines) and out.mod + out.readset written (mgReadsetWrite: modasm.c:108-126).  Both
 * passes sort the hits by mod on the GPU; the files are the reference's, byte for byte but for the addresses a .readset holds.
 *
 *   gcc -O2 -I include examples/clean_file.c -o clean_file -L modimizer_amd -lmodgpu -Wl,-rpath,$PWD/modimizer_amd -Wl,-rpath,/opt/rocm/lib
 *   ./clean_file stem [out]
 */
#include <stdio.h>
#include <stdlib.h>
#include "modgpu.h"

int main (int argc, char **argv)
{
  if (argc < 2) { fprintf (stderr, "usage: %s <stem of .mod + .readset> [stem to write]\n", argv[0]); return 2; }
  MgReadset *rs = mgReadsetLoad (argv[1]);                                             /* -r stem */
  Modset *ms = rs->ms; Seqhash *sh = ms->hasher;
  if (mgReadsetCleanMods (rs, stdout)) { fprintf (stderr, "FATAL ERROR: -C: %s\n", mgLastError ()); return 1; }      /* -C */
  if (mgReadsetProperties (rs, stdout)) { fprintf (stderr, "FATAL ERROR: -P: %s\n", mgLastError ()); return 1; }     /* -P */
  if (argc > 2) mgReadsetWrite (rs, argv[2]);                                          /* -w out */
  fprintf (stderr, "-C %s, -P %s\n", mgReadsetCleanModsPath () ? "by the host loops" : "on the device", mgReadsetPropertiesPath () ? "by the host loops" : "on the device");
  mgReadsetDestroy (rs);
  modsetDestroy (ms); mgSeqhashDestroy (sh);                                           /* mgReadsetLoad made both (modasm.c:100-107) */
  return 0;
}
