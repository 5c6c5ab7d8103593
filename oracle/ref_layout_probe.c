/* oracle/ref_layout_probe.c — TEST INFRASTRUCTURE ONLY (tests/test_dropin.py).
 *
 * oracle/Makefile `ref` compiles it against the reference's headers, where the reference tree is:
 *   -DLAYER2 -c          the reference's modset.h and seqio.h, then modgpu.h, in one translation unit -> _ref/layer2_header.o
 *   -DREF                the struct layouts the reference's modset.h declares                          -> _ref/ref_layout_probe
 * and the test compiles it against include/modgpu.h alone: both programs must print the same layouts. */
#ifdef LAYER2
#include "modset.h"
#include "seqio.h"
#include "modgpu.h"
I64 f (Modset *ms, char *b, int64_t *o, int n) { msSetCopy1 (ms, 1); return mgAddSequenceBatch (ms, b, o, n) + (I64) sizeof (MgReference); }
#else
#include <stdio.h>
#include <stddef.h>
#ifdef REF
#include "modset.h"
#else
#include "modgpu.h"
#endif
int main (void)
{ printf ("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof (Seqhash), sizeof (SeqhashRCiterator), sizeof (Modset),
          offsetof (Seqhash, factor1), offsetof (Seqhash, patternRC), offsetof (SeqhashRCiterator, hashBuf), offsetof (Modset, index), offsetof (Modset, max));
  return 0;
}
#endif
