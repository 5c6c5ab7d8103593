/* mg_readset_int.h — what the files of modasm's read set share with one another: mg_readset.c (the set itself, the ingest, the files),
 * mg_rs_clean.c (-C, -P), mg_rs_overlap.c (-o1, -o2, -b, -c), mg_rs_rdna.c (-R, -T, -rb).  Not installed, nothing in it is exported. */
#ifndef MG_READSET_INT_H
#define MG_READSET_INT_H
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"
#include "mg_internal.h"

#define TOPBIT  MG_TOPBIT          /* modasm.c:22: set for forward orientation */
#define TOPMASK MG_TOPMASK

/* a pass goes by its host loops: a set of 2^32 - 16 hits or more, or MODGPU_READSET_HOST=1 */
static inline int rsHostForced (const MgReadset *rs) { return rs->totHit >= 0xfffffff0ull || mgKnobs ()->readsetHost == 1; }
static inline int rsU32Cmp (const void *a, const void *b) { const U32 x = *(const U32 *) a, y = *(const U32 *) b; return x < y ? -1 : x > y; }

/* mg_readset.c */
MG_HIDDEN void mgRsViewOf (const MgReadset *rs, MgRsView *v);      /* the set as it is now, for a device entry point (run: 0) */
MG_HIDDEN U64  mgRsInvPlaces (const Modset *ms, U64 *invStart, const U64 *held);
MG_HIDDEN void mgRsInvBuildHost (MgReadset *rs, const char *root);
MG_HIDDEN int  mgRsCopyTallies (const MgReadset *rs, const U8 *info, int host, int *nc);
/* mg_rs_rdna.c: ModInfo, otherFlags and the -T count kept beside a set.  Forget: when the set goes; FlagsOf: otherFlags[0 .. nReads], 0 if there is
   none and create is 0 */
MG_HIDDEN void mgRsRdnaForget (const MgReadset *rs);
MG_HIDDEN U8  *mgRsRdnaFlagsOf (const MgReadset *rs, int create);
#endif
