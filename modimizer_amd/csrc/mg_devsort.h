/* mg_devsort.h — the device-wide primitives over U32 that the Reference's pack (mg_refpack.hip) and the read set's device passes
 * (mg_rsdev.hip) share: an exclusive scan and a stable radix sort (mg_devsort.hip).  Neither takes scratch from its caller. */
#ifndef MG_DEVSORT_H
#define MG_DEVSORT_H
#include "mg_common.h"

#define MG_SCAN_TILE  4096         /* elements per workgroup of a scan pass: 256 threads x 16 */
#define MG_RSORT_TILE 8192         /* elements per workgroup of a sort pass */

/* the bits of the keys 0 .. maxKey (at least 1, at most 32): what a sort by them has to look at */
int mgKeyBits (U64 maxKey);
/* words of scratch a scan of n elements takes from the owner: a bound for a caller that asks first whether the device has room */
size_t mgScanScratchWords (U64 n);
/* out[i] = sum of in[0 .. i) for i < n (in == out allowed; the sums stay below 2^32: they count occurrences).  total != 0: *total = the
   sum of all n, on the host, and the stream has been waited for */
MgStatus mgExclusiveScan (MgDevScratch &scratch, const U32 *in, U32 *out, U64 n, hipStream_t st, U32 *total = 0);
/* values (vals, or the positions 0 .. n-1 when vals == 0) in the order of their keys, equal keys in their original order: LSD passes of
   8 bits over keyBits bits.  *out: a fresh array of n + 1 words that scratch holds (scratch.take () hands it on); the stream has been waited for */
MgStatus mgRefStableSort (MgDevScratch &scratch, const U32 *keys, const U32 *vals, U32 n, int keyBits, U32 **out, hipStream_t st);
#endif
