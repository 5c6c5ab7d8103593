/* mg_gzipsrc.hip — an ordinary gzip file (gzip, pigz, zlib, an instrument's software: one member or several, no block table) as a source of text ON THE
 * DEVICE for the window loop (mgTextStreamWindowsDev), beside mg_bgzfsrc.hip and with its contract.
 *
 * Which files (mgGzipSrcOpen).  A regular file that begins 1f 8b 08, whose first member carries no 'BC' extra subfield (a file that is nearly BGZF keeps the
 * path it has), that is at least MODGPU_GZIP_MIN_KB in size and not more than the device keeps: the compressed file is uploaded ONCE -- read by the parser's
 * team of readers into page-locked pieces, one read while the piece before is on the link (MgDevFile, mg_devfile.h) -- and STAYS on the device, by the
 * rule of mgFileStays (8 GiB, a quarter of the free memory), so the call's second walk reads and uploads nothing.  A larger file is the host's, as before.
 *
 * Filling a window (mgGzipSrcFill).  The stream (mg_gunzip.hip) inflates a batch of chunks ahead of the windows into its own staging; a window is device-to-
 * device copies out of it, what a window leaves over stays there for the next one.  The text's length is not known before its last batch, so a full window
 * asks for the next batch before it says whether text follows.  The window's first and last byte are fetched (two bytes); no window comes back.
 * The chunks per batch are cut to what a quarter of the free device memory holds (symbols, text and windows: about three bytes a symbol).
 * A stream error fails the fill with the compressed file offset in the message, as a corrupt BGZF member does. */
#include <fcntl.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include "mg_common.h"
#include "mg_internal.h"
#include "mg_devfile.h"
#include "mg_gunzip_core.h"

#define GS_CHUNK_KB 64                                   /* the defaults are measured: DESIGN.md, "Ordinary gzip inflated on the device" */
#define GS_BATCH 4096
#define GS_MIN_KB 16384                                  /* below it one chunk's serial decode (about 0.1 s) is more than the host's whole inflate */
#define GS_MIN_KB_FLOOR 1024                             /* what the default is never set below: a file of a few chunks leaves the chip empty */

struct MgGzipSrc {
  std::string name; int fd = -1; U64 fileSize = 0, hint = 0;
  U32 chunkBytes = 0, batch = 0, spc = 0;
  unsigned char *dComp = 0; bool uploaded = false;
  MgGunzipDev *g = 0;
  const U8 *text = 0; size_t have = 0; int done = 0;
  U64 pos = 0;
  MgFillEdge edge;
};

static U64 gsMinBytes (void)
{
  const long v = mgKnobs ()->gzipMinKb;
  return (U64) (v == MG_KNOB_UNSET || v < 0 ? (GS_MIN_KB > GS_MIN_KB_FLOOR ? GS_MIN_KB : GS_MIN_KB_FLOOR) : v) << 10;
}

extern "C" int mgGzipSrcOpen (const char *name, int fd, U64 fileSize, int any, MgGzipSrc **out)
{
  *out = 0;
  const MgKnobs *kn = mgKnobs ();
  if (!any && (kn->gzipHost == 1 || fileSize < gsMinBytes ())) return -2;
  if (fileSize < 18 || fileSize > MG_FILE_RESIDENT_MAX) return -2;
  std::string head ((size_t) (fileSize < 70000 ? fileSize : 70000), '\0');
  if (pread (fd, &head[0], head.size (), 0) != (ssize_t) head.size ()) return -2;
  uint64_t len = 0; int bc = 0;
  if (mgzHeader ((const uint8_t *) head.data (), head.size (), &len, &bc) == 2 || bc) return -2;
  if (mgEnsureDevice () != MG_OK) return -1;
  size_t freeB = 0;
  if (!mgFileStays (fileSize, &freeB)) return -2;
  MgGzipSrc *s = new MgGzipSrc; s->name = name ? name : ""; s->fd = fd; s->fileSize = fileSize;
  unsigned char t[4] = { 0, 0, 0, 0 };
  (void) ! pread (fd, t, 4, (off_t) (fileSize - 4));
  const U64 isize = (U64) t[0] | ((U64) t[1] << 8) | ((U64) t[2] << 16) | ((U64) t[3] << 24);
  s->hint = isize > fileSize ? isize : fileSize * 4;      /* (one member below 4 GiB of text states its length; anything else: the guess a stream gets) */
  s->chunkBytes = (U32) (kn->gzipChunkKb == MG_KNOB_UNSET ? GS_CHUNK_KB : kn->gzipChunkKb < 4 ? 4 : kn->gzipChunkKb > (1 << 20) ? (1 << 20) : kn->gzipChunkKb) << 10;
  U64 ratio = kn->gzipRatio != MG_KNOB_UNSET && kn->gzipRatio > 0 ? (U64) kn->gzipRatio : isize > fileSize ? (isize * 3 / 2 + fileSize - 1) / fileSize + 1 : 8;
  if (ratio * s->chunkBytes > MGZ_SYM_MAX) ratio = MGZ_SYM_MAX / s->chunkBytes;
  s->spc = (U32) (ratio * s->chunkBytes);
  U64 batch = kn->gzipBatch != MG_KNOB_UNSET && kn->gzipBatch > 0 ? (U64) kn->gzipBatch : GS_BATCH;
  const U64 per = (U64) s->spc * 3 + MGZ_WINDOW + sizeof (MgzChunk), room = (freeB - fileSize) / 4;
  if (batch > room / per) batch = room / per;
  if (batch < 1) batch = 1;
  s->batch = (U32) (batch > 0x7fffffffu ? 0x7fffffffu : batch);
  *out = s;
  return 0;
}
extern "C" void mgGzipSrcClose (MgGzipSrc *s)
{
  if (!s) return;
  mgGunzipDevClose (s->g); (void) hipFree (s->dComp); s->edge.release ();
  delete s;
}
extern "C" void mgGzipSrcRewind (MgGzipSrc *s) { s->pos = 0; s->have = 0; s->text = 0; s->done = 0; if (s->g) mgGunzipDevRewind (s->g); }
extern "C" U64 mgGzipSrcSizeHint (const MgGzipSrc *s) { return s->hint; }

/* the compressed file to the device, once */
static int gsUpload (MgGzipSrc *s, hipStream_t st)
{
  const char *what = "gzip on the device";
  MgDevFile file;
  int rc = file.reserve ((size_t) s->fileSize, what);
  if (rc == -2 || (!rc && !s->edge.ready ())) { mgSetError ("gzip %s: no page-locked memory", s->name.c_str ()); rc = -1; }
  if (!rc && hipMalloc ((void **) &s->dComp, (size_t) s->fileSize) != hipSuccess) { mgHipFail (hipGetLastError (), what); rc = -1; }
  if (!rc && (rc = file.upload (s->fd, 0, (size_t) s->fileSize, s->dComp, st, what)) == -2) mgSetError ("failed to read sequence file %s", s->name.c_str ());
  if (hipStreamSynchronize (st) != hipSuccess && !rc) { mgHipFail (hipGetLastError (), what); rc = -1; }
  file.release ();
  if (rc) return -1;
  mgInflateDiagUploaded (s->fileSize);
  if (mgGunzipDevOpen (s->dComp, s->fileSize, s->fd, s->chunkBytes, s->batch, s->spc, &s->g)) return -1;
  s->uploaded = true;
  return 0;
}

/* text into the staging if it is empty and the stream has more; 0 / -1 */
static int gsAhead (MgGzipSrc *s, hipStream_t st)
{
  if (s->have || s->done) return 0;
  U32 status = 0; U64 errOff = 0;
  if (mgGunzipDevNext (s->g, (void *) st, &s->text, &s->have, &s->done, &status, &errOff))
    { if (status) mgSetError ("sequence file %s: corrupt gzip stream at file offset %llu (inflate status %u)", s->name.c_str (), (unsigned long long) errOff, status);
      return -1;
    }
  return 0;
}

extern "C" int mgGzipSrcFill (MgGzipSrc *s, unsigned char *dDst, size_t cap, U64 off, U64 limit, void *stream, size_t *n, int *more, U32 *first, U32 *last)
{
  hipStream_t st = (hipStream_t) stream;
  *n = 0; *more = 0; *first = *last = 0;
  size_t want = 0;
  if (mgFillWant ("gzip", s->name.c_str (), off, s->pos, limit, cap, &want)) return -1;
  if (!want) return 0;
  if (!s->uploaded && gsUpload (s, st)) return -1;
  size_t got = 0;
  while (got < want)
    { if (gsAhead (s, st)) { (void) hipStreamSynchronize (st); return -1; }
      if (!s->have) break;
      const size_t take = s->have < want - got ? s->have : want - got;
      if (hipMemcpyAsync (dDst + got, s->text, take, hipMemcpyDeviceToDevice, st) != hipSuccess) return mgHipFail (hipGetLastError (), "gzip on the device"), -1;
      s->text += take; s->have -= take; got += take;
    }
  if (!got) return 0;
  if (got == want && off + got < limit && gsAhead (s, st)) { (void) hipStreamSynchronize (st); return -1; }      /* does text follow? */
  if (s->edge.fetch ("gzip", dDst, got, st, first, last)) return -1;
  s->pos += got;
  *n = got; *more = s->have > 0 && s->pos < limit;
  return 0;
}
