/* mg_textsrc.h — where the text of a walk over mgTextStreamWindows comes from (mg_composition.hip, mg_seqconvert.hip; mg_filecodec.hip for its two device sources): the `src` and `fill` of that call */
#ifndef MG_TEXTSRC_H
#define MG_TEXTSRC_H
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include "mg_common.h"
#include "mg_knobs.h"
#include "mg_internal.h"

/* where the text comes from: a plain file (the parser's team of readers), blocked gzip or ordinary gzip inflated on the device, a stream the host inflates, host memory; at most `limit` bytes of it */
struct CpSource {
  const char *name = 0;
  int fd = -1; FILE *fz = 0;
  MgBgzfSrc *bz = 0;                /* blocked gzip from end to end: inflated on the device (mg_bgzfsrc.hip), fd stays open for its reads */
  MgGzipSrc *gz = 0;                /* ordinary gzip of a size the device takes: inflated there chunk by chunk (mg_gzipsrc.hip), fd stays open for its reads */
  const unsigned char *mem = 0;
  U64 size = 0;                     /* of the plain file / the memory; a guess for a stream */
  U64 limit = ~(U64) 0;
  bool stream () const { return fz != 0 || gz != 0; }      /* the text's size is a guess */
  int open (const char *filename)
  { name = filename;
    fd = ::open (filename, O_RDONLY);
    if (fd < 0) { mgSetError ("failed to open sequence file %s", filename); return -1; }
    struct stat sb; unsigned char magic[2] = { 0, 0 };
    const bool regular = fstat (fd, &sb) == 0 && S_ISREG (sb.st_mode);
    if (regular && sb.st_size == 0) { mgSetError ("sequence file %s unreadable or empty", filename); return -1; }
    if (regular && pread (fd, magic, 2, 0) == 2 && !(magic[0] == 0x1f && magic[1] == 0x8b)) { size = (U64) sb.st_size; return 0; }
    if (regular && mgKnobs ()->bgzfHost != 1)                  /* blocked gzip and nothing else: the device inflates (MODGPU_BGZF_HOST=1: the host, as below) */
      { const int rc = mgBgzfSrcOpen (filename, fd, (U64) sb.st_size, &bz);
        if (rc == -1) return -1;
        if (!rc) { size = mgBgzfSrcTextBytes (bz); return 0; }
      }
    if (regular)                                              /* ordinary gzip, large enough: the device inflates (MODGPU_GZIP_HOST=1, MODGPU_GZIP_MIN_KB: the host, as below) */
      { const int rc = mgGzipSrcOpen (filename, fd, (U64) sb.st_size, 0, &gz);
        if (rc == -1) return -1;
        if (!rc) { size = mgGzipSrcSizeHint (gz); return 0; }
      }
    ::close (fd); fd = -1;                                    /* gzip (the reference reads everything through gzread, seqio.c:33-40): the host inflates, the device counts */
    size = regular ? (U64) sb.st_size * 4 : (U64) 1 << 30;
    return reopen ();
  }
  int reopen ()
  { if (bz) { mgBgzfSrcRewind (bz); return 0; }
    if (gz) return mgGzipSrcRewind (gz);
    if (!name || fd >= 0) return 0;
    if (fz) fclose (fz);
    fz = mgFzOpen (name, "r");
    if (!fz) { mgSetError ("failed to open sequence file %s", name); return -1; }
    return 0;
  }
  void close () { if (bz) mgBgzfSrcClose (bz); bz = 0; if (gz) mgGzipSrcClose (gz); gz = 0; if (fd >= 0) ::close (fd); if (fz) fclose (fz); fd = -1; fz = 0; }
  static size_t fill (void *v, unsigned char *dst, size_t cap, U64 off)
  { CpSource *s = (CpSource *) v;
    if (off >= s->limit) return 0;
    if (s->limit - off < cap) cap = (size_t) (s->limit - off);
    if (s->fz) { const size_t g = fread (dst, 1, cap, s->fz); return g < cap && ferror (s->fz) ? (size_t) -1 : g; }
    if (off >= s->size) return 0;
    if (s->size - off < cap) cap = (size_t) (s->size - off);
    if (s->mem) { memcpy (dst, s->mem + off, cap); return cap; }
    return mgTextReadParallel (s->fd, dst, cap, (int64_t) off) ? (size_t) -1 : cap;
  }
  static int dfill (void *v, unsigned char *dDst, size_t cap, U64 off, void *stream, size_t *n, int *more, U32 *first, U32 *last)
  { CpSource *s = (CpSource *) v;
    if (s->gz) return mgGzipSrcFill (s->gz, dDst, cap, off, s->limit, stream, n, more, first, last);
    return mgBgzfSrcFill (s->bz, dDst, cap, off, s->limit, stream, n, more, first, last);
  }
  /* the walk over this source: the device fills the windows of a blocked-gzip or gzip file, `fill` (CpSource::fill or a wrapper of it) every other text's */
  int walk (size_t sizeHint, MgTextFillFn fillFn, MgTextWindowFn fn, void *ctx, U64 *nWindows)
  { return bz || gz ? mgTextStreamWindowsDev (sizeHint, dfill, this, fn, ctx, nWindows) : mgTextStreamWindows (sizeHint, fillFn, this, fn, ctx, nWindows); }
};
#endif
