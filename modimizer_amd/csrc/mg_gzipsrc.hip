/* mg_gzipsrc.hip — an ordinary gzip file (gzip, pigz, zlib, an instrument's software: one member or several, no block table) as a source of text ON THE
 * DEVICE for the window loop (mgTextStreamWindowsDev) and for the text parser (mg_textgpu.hip), beside mg_bgzfsrc.hip and with its contract.
 *
 * Which files (mgGzipSrcOpen).  A regular file that begins 1f 8b 08, whose first member carries no 'BC' extra subfield (a file that is nearly BGZF keeps the
 * path it has) and that is at least MODGPU_GZIP_MIN_KB in size.  Two modes:
 *   resident  (composition, seqconvert, mgGzipInflateFile: two walks).  The compressed file is uploaded ONCE -- read by the parser's team of readers into
 *             page-locked pieces, one read while the piece before is on the link (MgDevFile, mg_devfile.h) -- and STAYS on the device, by the rule of
 *             mgFileStays (8 GiB, a quarter of the free memory), so the call's second walk reads and uploads nothing.  A larger file is the host's.
 *   one walk  (MG_GZIP_ONE_WALK: the text parser, whose device memory is the modset table's).  Only a RANGE of the file is on the device: before every
 *             batch the stream (mg_gunzip.hip) asks for the bytes from the batch's first on, the range takes them up in whole pieces behind what it
 *             holds, and what lies before the batch's start is given up -- every byte is uploaded exactly once, the file's size does not matter, and
 *             neither limit of mgFileStays applies.  The kernels address the file by absolute offset, so they get the range's base moved back by the
 *             range's first offset and the range's end as the bytes' end.  The range lives in a block of twice its span, so that giving up the front is
 *             one copy between parts that do not overlap.  Its bound (mgGzipSrcDiag) follows from chunk bytes, chunks a batch and the piece; a block
 *             that no range of that size holds (a stored block of 65 535 bytes against chunks of 4 KiB) makes the stream ask for twice the span.
 *
 * Filling a window (mgGzipSrcFill).  The stream inflates a batch of chunks ahead of the windows into its own staging; a window is device-to-
 * device copies out of it, what a window leaves over stays there for the next one.  The text's length is not known before its last batch, so a full window
 * asks for the next batch before it says whether text follows.  The window's first and last byte are fetched (two bytes); no window comes back.
 * The chunks per batch are cut to what a quarter of the free device memory holds (symbols, text and windows: about three bytes a symbol).
 * A stream error fails the fill with the compressed file offset in the message, as a corrupt BGZF member does. */
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>
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
  int first = -1;                                        /* the text's first byte, from the file's head inflated on the host; -1: the head does not say */
  unsigned char *dComp = 0; bool uploaded = false;       /* resident: the whole file */
  bool oneWalk = false;                                  /* one walk: file bytes [lo, hi) at dRange[0 .. hi - lo), in a block of cap bytes */
  unsigned char *dRange = 0; U64 cap = 0, lo = 0, hi = 0; MgDevFile file;
  MgGunzipDev *g = 0;
  const U8 *text = 0; size_t have = 0; int done = 0;
  U64 pos = 0;
  MgFillEdge edge;
};

/* of the calling thread's last one-walk source (mgGzipSrcDiag): bytes uploaded, refills, the most compressed bytes resident at once, the bound */
static thread_local U64 gGsDiag[4];
extern "C" void mgGzipSrcDiag (U64 out4[4]) { memcpy (out4, gGsDiag, sizeof (gGsDiag)); }

static U64 gsMinBytes (void)
{
  const long v = mgKnobs ()->gzipMinKb;
  return (U64) (v == MG_KNOB_UNSET || v < 0 ? (GS_MIN_KB > GS_MIN_KB_FLOOR ? GS_MIN_KB : GS_MIN_KB_FLOOR) : v) << 10;
}

/* the span a batch of full size asks for -- its chunks and one more, where the last chunk's decode runs on to a block boundary -- with the piece the
   range's upload is rounded up by; the range's block is twice that */
static U64 gsSpan (const MgGzipSrc *s) { return ((U64) s->batch + 1) * s->chunkBytes + mgFilePieceBytes (); }
static U64 gsBound (const MgGzipSrc *s) { return 2 * gsSpan (s); }

/* the first byte of the text of the gzip file that begins with head[0 .. n): zlib on the host, over empty members; -1 if the head does not hold it */
extern "C" int mgGzipFirstByte (const unsigned char *head, size_t n)
{
  z_stream zs; memset (&zs, 0, sizeof (zs));
  if (inflateInit2 (&zs, 15 + 16) != Z_OK) return -1;
  unsigned char out = 0;
  zs.next_in = (Bytef *) head; zs.avail_in = (uInt) n; zs.next_out = &out; zs.avail_out = 1;
  int first = -1;
  for (;;)
    { const int rc = inflate (&zs, Z_NO_FLUSH);
      if (!zs.avail_out) { first = out; break; }
      if (rc != Z_STREAM_END || !zs.avail_in || inflateReset (&zs) != Z_OK) break;      /* (an empty member: the next one) */
    }
  inflateEnd (&zs);
  return first;
}

extern "C" int mgGzipSrcOpen (const char *name, int fd, U64 fileSize, int flags, MgGzipSrc **out)
{
  *out = 0;
  const MgKnobs *kn = mgKnobs ();
  const bool oneWalk = (flags & MG_GZIP_ONE_WALK) != 0;
  if (!(flags & MG_GZIP_ANY) && (kn->gzipHost == 1 || fileSize < gsMinBytes ())) return -2;
  if (fileSize < 18 || (!oneWalk && fileSize > MG_FILE_RESIDENT_MAX)) return -2;
  std::string head ((size_t) (fileSize < 70000 ? fileSize : 70000), '\0');
  if (pread (fd, &head[0], head.size (), 0) != (ssize_t) head.size ()) return -2;
  uint64_t len = 0; int bc = 0;
  if (mgzHeader ((const uint8_t *) head.data (), head.size (), &len, &bc) == 2 || bc) return -2;
  if (mgEnsureDevice () != MG_OK) return -1;
  size_t freeB = 0;
  if (oneWalk) (void) mgDevFreeBytes (&freeB);
  else if (!mgFileStays (fileSize, &freeB)) return -2;
  MgGzipSrc *s = new MgGzipSrc; s->name = name ? name : ""; s->fd = fd; s->fileSize = fileSize; s->oneWalk = oneWalk;
  s->first = mgGzipFirstByte ((const unsigned char *) head.data (), head.size ());
  unsigned char t[4] = { 0, 0, 0, 0 };
  (void) ! pread (fd, t, 4, (off_t) (fileSize - 4));
  const U64 isize = (U64) t[0] | ((U64) t[1] << 8) | ((U64) t[2] << 16) | ((U64) t[3] << 24);
  s->hint = isize > fileSize ? isize : fileSize * 4;      /* (one member below 4 GiB of text states its length; anything else: the guess a stream gets) */
  s->chunkBytes = (U32) (kn->gzipChunkKb == MG_KNOB_UNSET ? GS_CHUNK_KB : kn->gzipChunkKb < 4 ? 4 : kn->gzipChunkKb > (1 << 20) ? (1 << 20) : kn->gzipChunkKb) << 10;
  U64 ratio = kn->gzipRatio != MG_KNOB_UNSET && kn->gzipRatio > 0 ? (U64) kn->gzipRatio : isize > fileSize ? (isize * 3 / 2 + fileSize - 1) / fileSize + 1 : 8;
  if (ratio * s->chunkBytes > MGZ_SYM_MAX) ratio = MGZ_SYM_MAX / s->chunkBytes;
  s->spc = (U32) (ratio * s->chunkBytes);
  U64 batch = kn->gzipBatch != MG_KNOB_UNSET && kn->gzipBatch > 0 ? (U64) kn->gzipBatch : GS_BATCH;
  const U64 perFile = oneWalk ? 2 * s->chunkBytes : 0;   /* one walk: the range's block takes two bytes per chunk byte, the whole file's bytes at the most */
  const U64 per = (U64) s->spc * 3 + MGZ_WINDOW + sizeof (MgzChunk) + perFile, room = (oneWalk ? freeB : freeB - fileSize) / 4;
  if (batch > room / per) batch = room / per;
  if (batch < 1) batch = 1;
  s->batch = (U32) (batch > 0x7fffffffu ? 0x7fffffffu : batch);
  if (oneWalk) { memset (gGsDiag, 0, sizeof (gGsDiag)); gGsDiag[3] = gsBound (s); }
  *out = s;
  return 0;
}
extern "C" void mgGzipSrcClose (MgGzipSrc *s)
{
  if (!s) return;
  mgGunzipDevClose (s->g); (void) hipFree (s->dComp); (void) hipFree (s->dRange); s->file.release (); s->edge.release ();
  delete s;
}
extern "C" int mgGzipSrcRewind (MgGzipSrc *s)
{
  if (s->oneWalk) { mgSetError ("gzip %s: a source opened for one walk cannot be rewound", s->name.c_str ()); return -1; }
  s->pos = 0; s->have = 0; s->text = 0; s->done = 0; if (s->g) mgGunzipDevRewind (s->g);
  return 0;
}
extern "C" U64 mgGzipSrcSizeHint (const MgGzipSrc *s) { return s->hint; }
extern "C" int mgGzipSrcFirstByte (const MgGzipSrc *s) { return s->first; }

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

/* One walk: the stream is about to read file bytes [from, to) (MgGunzipRangeFn).  What the range holds before `from` is given up, the file is taken up
   behind the range's end in whole pieces until it reaches `to`, by copies on `stream`; *comp + o is the file's byte o for every o in the range, *end
   the range's end.  0, -1 with the error set */
static int gsRange (void *v, U64 from, U64 to, void *stream, const U8 **comp, U64 *end)
{
  MgGzipSrc *s = (MgGzipSrc *) v;
  hipStream_t st = (hipStream_t) stream;
  const char *what = "gzip on the device";
  const U64 piece = mgFilePieceBytes ();
  if (from > s->hi) from = s->hi;                        /* (a trailer and a header the host read lie between: they are taken up with the rest, every byte once) */
  if (to > s->fileSize) to = s->fileSize;
  if (from < s->lo) { mgSetError ("gzip %s: byte %llu asked for, given up at byte %llu", s->name.c_str (), (unsigned long long) from, (unsigned long long) s->lo); return -1; }
  U64 upTo = s->hi;
  if (to > upTo) { upTo += (to - upTo + piece - 1) / piece * piece; if (upTo > s->fileSize) upTo = s->fileSize; }
  if (upTo - s->lo > s->cap)                             /* the block's end is reached: the bytes still wanted go to the front of it, or of a larger one */
    { U64 want = 2 * (upTo - from);
      if (want < gsBound (s)) want = gsBound (s);
      if (want > s->fileSize) want = s->fileSize;
      const U64 live = s->hi - from, at = from - s->lo;
      if (want <= s->cap && live <= at)
        { if (live && hipMemcpyAsync (s->dRange, s->dRange + at, (size_t) live, hipMemcpyDeviceToDevice, st) != hipSuccess) return mgHipFail (hipGetLastError (), what), -1; }
      else
        { unsigned char *grown = 0;
          if (want < s->cap) want = s->cap;
          if (hipMalloc ((void **) &grown, (size_t) want) != hipSuccess) return mgHipFail (hipGetLastError (), what), -1;
          if ((live && hipMemcpyAsync (grown, s->dRange + at, (size_t) live, hipMemcpyDeviceToDevice, st) != hipSuccess) || hipStreamSynchronize (st) != hipSuccess)
            { mgHipFail (hipGetLastError (), what); (void) hipFree (grown); return -1; }
          (void) hipFree (s->dRange);
          s->dRange = grown; s->cap = want;
        }
      s->lo = from;
    }
  if (upTo > s->hi)
    { const int rc = s->file.upload (s->fd, s->hi, (size_t) (upTo - s->hi), s->dRange + (s->hi - s->lo), st, what);
      if (rc == -2) mgSetError ("failed to read sequence file %s", s->name.c_str ());
      if (rc) return -1;
      mgInflateDiagUploaded (upTo - s->hi);
      gGsDiag[0] += upTo - s->hi; ++gGsDiag[1];
      s->hi = upTo;
    }
  if (s->hi - s->lo > gGsDiag[2]) gGsDiag[2] = s->hi - s->lo;
  *comp = (const U8 *) ((uintptr_t) s->dRange - (uintptr_t) s->lo);
  *end = s->hi;
  return 0;
}
static int gsOpenWalk (MgGzipSrc *s)
{
  const int rc = s->file.reserve ((size_t) s->fileSize, "gzip on the device");
  if (rc == -2 || (!rc && !s->edge.ready ())) { mgSetError ("gzip %s: no page-locked memory", s->name.c_str ()); return -1; }
  if (rc || mgGunzipDevOpen (0, s->fileSize, s->fd, s->chunkBytes, s->batch, s->spc, &s->g)) return -1;
  mgGunzipDevRange (s->g, gsRange, s);
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
  if (!s->uploaded && (s->oneWalk ? gsOpenWalk (s) : gsUpload (s, st))) return -1;
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
