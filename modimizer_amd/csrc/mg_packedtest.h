/* mg_packedtest.h — "which bytes of a word are below N", for four values packed into one register: the FAST scan filter's threshold
 * test for four k-mer starts at once (mg_scan.hip, phase A).  Plain C: the kernel and the host (the library's test hook
 * mgScanBytesBelow) compile the same line.
 *
 * acc holds four bytes, nRep = 0x01010101 * N with 1 <= N <= 32.  Bit 8j + 7 of the result is set
 *   - for every byte j below N (its difference borrows, its own top bit is clear: N <= 128 would do for this half), and
 *   - for a byte j that EQUALS N when byte j - 1 borrowed, i.e. was itself flagged (the borrow of the word-wide subtraction runs into
 *     it) -- and for no other byte.
 * So the flags are a superset of the bytes below N: what the filter needs, since every candidate it passes is evaluated exactly. */
#ifndef MG_PACKEDTEST_H
#define MG_PACKEDTEST_H
#include <stdint.h>
#if defined (__HIPCC__) || defined (__CUDACC__)
#define MG_PT_BOTH __host__ __device__
#else
#define MG_PT_BOTH
#endif
#define MG_PT_TOPS 0x80808080u
MG_PT_BOTH static inline uint32_t mgBytesBelow (uint32_t acc, uint32_t nRep) { return (acc - nRep) & ~acc & MG_PT_TOPS; }
/* nRep for the filter of d = 2^dShift, 3 <= dShift <= 8: min (hf, hr) < 2^(32 - dShift)  <=>  its top byte < 2^(8 - dShift) */
MG_PT_BOTH static inline uint32_t mgBytesBelowRep (int dShift) { return 0x01010101u << (8 - dShift); }
#endif
