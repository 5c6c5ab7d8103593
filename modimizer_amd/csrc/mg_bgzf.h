/* mg_bgzf.h -- the header of a blocked-gzip (BGZF: bgzip, htslib) member, read in one place: by the host reader (mg_seqio.c) and by the
 * walk that hands a whole file's members to the device (mg_bgzfsrc.hip).  A member is a gzip member with FLG = FEXTRA whose extra field
 * holds a 'BC' subfield of 2 bytes: the member's size - 1.  Its deflate payload follows the extra field; CRC-32 and ISIZE end it. */
#ifndef MG_BGZF_H
#define MG_BGZF_H
#include <stddef.h>
static size_t bgzfBlockSize (const unsigned char *p, size_t avail, size_t *payloadOff)     /* 0: not a block header */
{
  if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0;
  const size_t xlen = (size_t) p[10] | ((size_t) p[11] << 8);
  if (avail < 12 + xlen) return 0;
  for (size_t at = 12 ; at + 4 <= 12 + xlen ; )
    { const size_t len = (size_t) p[at + 2] | ((size_t) p[at + 3] << 8);
      if (p[at] == 'B' && p[at + 1] == 'C' && len == 2 && at + 6 <= 12 + xlen)
        { *payloadOff = 12 + xlen; return ((size_t) p[at + 4] | ((size_t) p[at + 5] << 8)) + 1; }
      at += 4 + len;
    }
  return 0;
}
#endif
