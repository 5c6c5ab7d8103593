/* mg_modsettext.c — a set as text: modutils "-wt" (modutils.c:194-198) and "-rt" (modutils.c:169-190).
 * The dump is the host's; a regular file is read on the device (mg_settext.hip), an irregular one by the reference's own fscanf format here.
 */
#define _GNU_SOURCE
#include <stdlib.h>
#include <stdarg.h>
#include <string.h>
#include "modgpu.h"
#include "mg_internal.h"

void mgModsetWriteText (Modset *ms, FILE *f)
{
  if (modsetSyncToHost (ms, 0)) mgFatal ("modsetSyncToHost");
  Seqhash *sh = ms->hasher;
  fprintf (f, "modset bits %d size %d k %d w %d seed %d\n", ms->tableBits, ms->max + 1, sh->k, sh->w, sh->seed);
  for (U32 i = 1 ; i <= ms->max ; ++i)
    fprintf (f, "%d\t%s\t%d\t%d\n", (int) i, seqString (ms->value[i], sh->k), ms->depth[i], ms->info[i]);
}

/* modutils.c:169-190 ("-rt").  The header, the checks seqhashCreate / modsetCreate would die() on, the choice of the path and the
 * irregular file are the host's; the regular file is parsed and the set filled on the device (mg_settext.hip).  The host parser is the
 * reference's fscanf format itself, with %ms for its %s into a static char[33]: a token of more than 32 bytes, which overruns that
 * buffer there (undefined behaviour), is "bad line N" here. */
static __thread int gReadTextPath = -1;
int mgModsetReadTextPath (void) { return gReadTextPath; }

static void readTextError (const char *fmt, ...)
{ char buf[1024]; va_list ap; va_start (ap, fmt); vsnprintf (buf, sizeof (buf), fmt, ap); va_end (ap); mgSetErrorText (buf); }

/* lines 2 .. of the file by the reference's loop (modutils.c:181-184) into arrays; 0, or -1 with "bad line N" set.  *wide: some value is 4^k or more */
static int readTextHostLines (FILE *f, int n, int k, U64 *key, U16 *depth, U8 *info, int *wide)
{
  U64 conv[256]; memset (conv, 0, sizeof (conv));
  conv['c'] = conv['C'] = 1; conv['g'] = conv['G'] = 2; conv['t'] = conv['T'] = 3;
  *wide = 0;
  for (int i = 0 ; i < n ; ++i)
    { int ii, d, fl; char *seq = 0;
      const int got = fscanf (f, "%d\t%ms\t%d\t%d\n", &ii, &seq, &d, &fl);
      if (got != 4 || strlen (seq) > 32) { free (seq); readTextError ("bad line %d", 2 + i); return -1; }
      U64 x = 0;
      for (const unsigned char *c = (const unsigned char *) seq ; *c ; ++c) x = (x << 2) | conv[*c];
      free (seq);
      if (k < 32 && (x >> (2 * k))) *wide = 1;
      key[i] = x; depth[i] = (U16) d; info[i] = (U8) fl;
    }
  return 0;
}

Modset *mgModsetReadText (const char *filename)
{
  gReadTextPath = -1;
  if (!filename) { mgSetErrorText ("mgModsetReadText: invalid arguments"); return 0; }
  FILE *f = fopen (filename, "r");
  if (!f) { readTextError ("failed to open text file %s", filename); return 0; }
  int bits, size, k, w, seed;
  if (fscanf (f, "modset bits %d size %d k %d w %d seed %d\n", &bits, &size, &k, &w, &seed) != 5)
    { fclose (f); readTextError ("failed to read first line of text file %s\n", filename); return 0; }
  const long bodyOff = ftell (f);
  /* seqhash.c:22-23, modset.c:17,25, before anything is made */
  if (k < 1 || k >= 32) { fclose (f); readTextError ("seqhash k %d must be between 1 and 32\n", k); return 0; }
  if (w < 1) { fclose (f); readTextError ("seqhash w %d must be positive\n", w); return 0; }
  if (bits < 20 || bits > 34) { fclose (f); readTextError ("table bits %d must be between 20 and 34", bits); return 0; }
  if ((U32) size >= (((U64) 1 << bits) >> 2)) { fclose (f); readTextError ("Modset size %u is too big for %d bits", (U32) size, bits); return 0; }
  if (mgIterRequireDevice ()) { fclose (f); return 0; }
  const int n = size - 1 > 0 ? size - 1 : 0;              /* modutils.c:181: `i < size-1` in int arithmetic */
  Seqhash *sh = seqhashCreate (k, w, seed);
  Modset *ms = modsetCreate (sh, bits, (U32) size);
  ms->value[0] = 0;                                       /* (no entry: modsetCreate leaves it as malloc () gave it, and modsetWrite writes it) */
  int ok = 0;
  U64 *dKey = 0; U16 *dDepth = 0; U8 *dInfo = 0;
  const int dev = bodyOff < 0 ? 1 : mgSetTextParseDevice (filename, (U64) bodyOff, (U64) n, k, &dKey, &dDepth, &dInfo);
  if (dev == 0)
    { gReadTextPath = 0;
      ok = !mgSetTextFillDevice (ms, dKey, dDepth, dInfo, (U64) n);
      mgDeviceFree (dKey); mgDeviceFree (dDepth); mgDeviceFree (dInfo);
    }
  else if (dev == 1)
    { U64 *key = (U64 *) malloc ((size_t) n * 8 + 8); U16 *depth = (U16 *) malloc ((size_t) n * 2 + 8); U8 *info = (U8 *) malloc ((size_t) n + 8);
      if (!key || !depth || !info) mgFatal ("out of memory");
      int wide = 0;
      if (!readTextHostLines (f, n, k, key, depth, info, &wide))
        { if (!wide) { gReadTextPath = 1; ok = !mgSetTextFillHostArrays (ms, key, depth, info, (U64) n); }
          else
            { /* a value of 4^k or more may not enter a device table: the host algorithm (modutils.c:185-186), and the set stays on the host */
              gReadTextPath = 2;
              for (int i = 0 ; i < n ; ++i)
                { const U32 index = modsetIndexFind (ms, key[i], true);
                  ms->value[index] = key[i]; ms->depth[index] = depth[i]; ms->info[index] = info[i];
                }
              ok = 1;
            }
        }
      free (key); free (depth); free (info);
    }
  fclose (f);
  if (!ok) { modsetDestroy (ms); mgSeqhashDestroy (sh); return 0; }
  return ms;
}
