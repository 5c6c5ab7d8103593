/* mg_modrep_int.h — what the two modrep files share: mg_modrep.hip (-R, -s3, the per-read pass that -s1 reuses) and mg_modrep1.hip
 * (the end of a -s1 file, -s2).  Not part of the public ABI. */
#ifndef MG_MODREP_INT_H
#define MG_MODREP_INT_H
#include <stdlib.h>
#include <vector>
#include "mg_common.h"
#include "mg_internal.h"

#define MG_REP_FILE_BATCH 128000000ll      /* bases per batch of a file */

/* a file's run (modgpu.h): the per-read verdicts on the host, the hits of the good reads on the device, in (read, position) order */
struct MgRepRun {
  MgRepRef *ref = 0; Modset *ms = 0; int device = 0;
  MgDevBuf<U8> refIsF;                                /* ref->isF[0 .. max] */
  MgDevBuf<U32> hitK, hitX, hitRead; U64 nHit = 0;    /* the file's hits so far: modset index, position in the oriented read, good read ordinal */
  std::vector<int> n, seqF, seqR; std::vector<U8> bad, isF;      /* per read */
  std::vector<int> goodI, goodLen; std::vector<U64> hitStart;      /* per good read; hitStart: one more entry */
  int nBad = 0;
  ~MgRepRun () { refIsF.drop (); hitK.drop (); hitX.drop (); hitRead.drop (); }
};

/* the modimizers of a device batch scanned with scanWith (0: the set's own hasher), in (read, pos) order, and their indices in ms (0: absent):
   the library's seed list (mgSeedsOfBatch) from modrep's own first guess, its arrays handed to the scratch */
struct MgRepSeeds : MgSeedBufs { U64 n; };
MG_HIDDEN MgStatus mgRepSeedList (MgDevScratch &scratch, Modset *ms, const Seqhash *scanWith, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, MgRepSeeds *o, hipStream_t st);
/* host bases -> packed words and offsets in the scratch */
MG_HIDDEN MgStatus mgRepUpload (MgDevScratch &scratch, const char *bases, const int64_t *offsets, U32 nReads, U64 total, U32 **dPacked, U64 **dOff, hipStream_t st);
/* a .mod file, gzip or plain: 0 with the program's message if it cannot be opened */
MG_HIDDEN Modset *mgRepReadSet (const char *modFile);
MG_HIDDEN void mgRepSetDestroy (Modset *ms);
MG_HIDDEN void mgRepPathSet (int path);      /* what mgRepPath () answers on the calling thread */

/* a malloc ()ed copy of v with one spare element */
template <class T, class S> static T *mgRepCopyOut (const std::vector<S> &v)
{
  T *p = (T *) malloc ((v.size () + 1) * sizeof (T));
  if (p) for (size_t i = 0 ; i < v.size () ; ++i) p[i] = (T) v[i];
  return p;
}
#endif
