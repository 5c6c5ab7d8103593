/* mg_bgzfsrc.hip — a blocked-gzip (BGZF) file as a source of text ON THE DEVICE for the window loop (mgTextStreamWindowsDev):
 * the host walks the members' headers once, the compressed bytes cross the link, the kernel of mg_inflate.hip inflates them, and the
 * text lands in the window's device buffer.  No window comes back: the consumers get the window's first and last byte (two bytes).
 *
 * The walk (bzWalk).  A file is taken only if it is, from its first byte to its last, well-formed members with a 'BC' extra field
 * (bgzfBlockSize, mg_bgzf.h), each at most 64 KiB inflated; empty members (bgzip's end marker) are fine anywhere.  Anything else --
 * ordinary gzip, BGZF followed by an ordinary member, mg_pgzip.c's 16 MiB members, a truncated last block, a pipe -- is not this file's
 * business (-2), and the caller reads it as before.  One pread per member covers its trailer and the next header, which lie side by side.
 *
 * Filling a window (mgBgzfSrcFill).  Members do not align with windows, so members are inflated into a staging buffer of the source's
 * own -- eight windows and 64 KiB, 256 MiB at most: a launch over one window's members alone leaves most CUs without a wave -- and the
 * window is a device-to-device copy out of it; what a window leaves over stays there -- the tail is
 * carried on the device -- and moves to the front of the other staging buffer when more members are needed.  Members are taken in
 * batches whose compressed bytes, a contiguous stretch of the file with headers and trailers, are read by the parser's team of readers
 * into page-locked pieces, one read while the one before is on the link (MgDevFile, mg_devfile.h), and uploaded once.  Where device memory allows, the compressed file STAYS on the device
 * for the call's second walk (seqconvert's, composition's re-walk up to a cut): that walk reads and uploads nothing.  A caller that walks the
 * file once (the text parser, mg_textgpu.hip) says so (mgBgzfSrcOneWalk): nothing stays then, the compressed bytes pass through a ring of
 * look + 2 x 64 KiB, and the memory a resident file would take is the modset table's.
 * Everything runs on the stream the loop passes (its copy stream); the fill returns with the work over, the statuses checked and the
 * two bytes fetched, while the window before is still in its consumer's kernels. */
#include <fcntl.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <vector>
#include "mg_common.h"
#include "mg_internal.h"
#include "mg_devfile.h"
#include "mg_bgzf.h"

#define BZ_MEMBER 65536u                                 /* the most a member inflates to, and the most it occupies in the file */
#define BZ_LOOK_MAX ((size_t) 256 << 20)                 /* text inflated ahead of the windows: eight windows, this much at most (a window if it is larger) */

struct MgBgzfSrc {
  std::string name; int fd = -1; U64 fileSize = 0, textBytes = 0;
  std::vector<MgGzMember> mem;                           /* cOff: the payload's FILE offset; uOff: the member's offset in the text */
  std::vector<U64> start;                                /* the member's first byte in the file; [n] = fileSize */
  /* device side, made by the first fill */
  unsigned char *dStage[2] = { 0, 0 }; size_t stageCap = 0; int p = 0; size_t at = 0, have = 0;
  size_t look = 0;                                       /* text the staging buffer is filled up to: several windows, so that a launch has members for every CU */
  unsigned char *dComp = 0; size_t compCap = 0; bool resident = false; U64 uploadedTo = 0;
  bool oneWalk = false;                                  /* the caller walks the file once: the compressed bytes pass through a ring of look + 2 x 64 KiB, nothing stays */
  MgDevFile file;                                        /* the file crosses in pieces: one is read while the one before it is on the link */
  MgDevBuf<unsigned char> work; MgFillEdge edge;
  std::vector<MgGzMember> batch; std::vector<U32> status;
  size_t m = 0; U64 pos = 0;                             /* the next member to inflate; the text handed out so far */
  void release ()
  { for (int i = 0 ; i < 2 ; ++i) { (void) hipFree (dStage[i]); dStage[i] = 0; }
    (void) hipFree (dComp); dComp = 0; file.release (); edge.release (); work.drop ();
    stageCap = compCap = look = 0; resident = false; uploadedTo = 0;
  }
};

static U32 bzLe32 (const unsigned char *q) { return (U32) q[0] | ((U32) q[1] << 8) | ((U32) q[2] << 16) | ((U32) q[3] << 24); }

/* the member table of the whole file; 0, -2 = not BGZF from end to end */
static int bzWalk (MgBgzfSrc *s)
{
  unsigned char buf[8 + 64];
  U64 at = 0, text = 0;
  ssize_t g = pread (s->fd, buf + 8, 64, 0);
  while (at < s->fileSize)
    { size_t pay = 0;
      if (g < 18) return -2;
      const size_t size = bgzfBlockSize (buf + 8, (size_t) g, &pay);
      if (!size || size < pay + 8 + 2 || size > s->fileSize - at) return -2;      /* (a deflate stream is 2 bytes at least) */
      g = pread (s->fd, buf, sizeof (buf), (off_t) (at + size - 8));              /* this member's trailer and the next one's header */
      if (g < 8) return -2;
      MgGzMember k; memset (&k, 0, sizeof (k));
      k.cOff = at + pay; k.cLen = (U32) (size - pay - 8); k.crc = bzLe32 (buf); k.uLen = bzLe32 (buf + 4); k.uOff = text;
      if (k.uLen > BZ_MEMBER) return -2;
      s->mem.push_back (k); s->start.push_back (at);
      text += k.uLen; at += size; g -= 8;
    }
  if (s->mem.empty ()) return -2;
  s->start.push_back (s->fileSize); s->textBytes = text;
  return 0;
}

extern "C" int mgBgzfSrcOpen (const char *name, int fd, U64 fileSize, MgBgzfSrc **out)
{
  *out = 0;
  MgBgzfSrc *s = new MgBgzfSrc; s->name = name ? name : ""; s->fd = fd; s->fileSize = fileSize;
  const int rc = bzWalk (s);
  if (rc) { delete s; return rc; }
  *out = s;
  return 0;
}
extern "C" void mgBgzfSrcClose (MgBgzfSrc *s) { if (s) { s->release (); delete s; } }
extern "C" void mgBgzfSrcRewind (MgBgzfSrc *s) { s->m = 0; s->pos = 0; s->at = s->have = 0; }
extern "C" U64 mgBgzfSrcTextBytes (const MgBgzfSrc *s) { return s->textBytes; }
extern "C" void mgBgzfSrcOneWalk (MgBgzfSrc *s) { s->oneWalk = true; }      /* (before the first fill) */

/* member m inflated on the host (the decoder's host compile) behind what `text` holds; 0, -2 = it does not inflate */
static int bzHostMember (MgBgzfSrc *s, size_t m, std::vector<unsigned char> &comp, std::vector<unsigned char> &text)
{
  const MgGzMember &g = s->mem[m];
  comp.resize (g.cLen);
  if (pread (s->fd, comp.data (), g.cLen, (off_t) g.cOff) != (ssize_t) g.cLen) return -2;
  const size_t at = text.size (); text.resize (at + g.uLen);
  U32 status = 0;
  if (mgInflateMemberHost (comp.data (), g.cLen, text.data () + at, g.uLen, g.crc, &status, 0) || status) return -2;
  return 0;
}
/* what the text parser looks at before it starts, from the member table: the text's first byte, and its last min (cap, text) bytes into tail
   (*tailN of them) -- the first non-empty member and the last non-empty ones, walking back until the tail is in hand, inflated on the host.
   0, -2 = a member among them does not inflate (the caller leaves the file to the host reader, which reports it) */
extern "C" int mgBgzfSrcEdges (MgBgzfSrc *s, unsigned char *first, unsigned char *tail, size_t cap, size_t *tailN)
{
  *tailN = 0; *first = 0;
  if (!s->textBytes) return 0;
  std::vector<unsigned char> comp, text, piece;
  size_t m = 0;
  while (!s->mem[m].uLen) ++m;
  if (bzHostMember (s, m, comp, text)) return -2;
  *first = text[0];
  const size_t want = s->textBytes < cap ? (size_t) s->textBytes : cap;
  text.clear ();
  for (size_t k = s->mem.size () ; k-- > 0 && text.size () < want ; )
    { if (!s->mem[k].uLen) continue;
      piece.clear ();
      if (bzHostMember (s, k, comp, piece)) return -2;
      text.insert (text.begin (), piece.begin (), piece.end ());
    }
  memcpy (tail, text.data () + (text.size () - want), want);
  *tailN = want;
  return 0;
}

/* the first byte of a file's text: the file's own first byte, or for a file that starts with blocked-gzip members the first byte of the first
   non-empty one, inflated on the host; -1: none to be had (for a caller that picks its path by the format's first letter: mg_seqfiles.c) */
extern "C" int mgTextFirstByte (const char *filename)
{
  const int fd = open (filename, O_RDONLY);
  if (fd < 0) return -1;
  std::vector<unsigned char> buf (BZ_MEMBER + 64), text;
  int first = -1;
  for (U64 at = 0 ; ; )
    { const ssize_t g = pread (fd, buf.data (), buf.size (), (off_t) at);
      if (g < 1) break;
      size_t pay = 0;
      const size_t size = g >= 18 ? bgzfBlockSize (buf.data (), (size_t) g, &pay) : 0;
      if (!size)                                            /* plain text, ordinary gzip (or something the host reader judges) */
        { if (!at) first = g >= 3 && buf[0] == 0x1f && buf[1] == 0x8b && buf[2] == 8 ? mgGzipFirstByte (buf.data (), (size_t) g) : buf[0];
          break;
        }
      if (size < pay + 8 + 2 || size > (size_t) g) break;
      const U32 crc = bzLe32 (buf.data () + size - 8), uLen = bzLe32 (buf.data () + size - 4);
      if (uLen > BZ_MEMBER) break;
      if (!uLen) { at += size; continue; }
      text.resize (uLen);
      U32 status = 0;
      if (!mgInflateMemberHost (buf.data () + pay, (U32) (size - pay - 8), text.data (), uLen, crc, &status, 0) && !status) first = text[0];
      break;
    }
  close (fd);
  return first;
}

static int bzReserve (MgBgzfSrc *s, size_t cap)
{
  if (s->stageCap >= cap + BZ_MEMBER && s->look >= cap) return 0;
  if (s->have) { mgSetError ("blocked gzip %s: the window grew in the middle of a walk", s->name.c_str ()); return -1; }
  s->release ();
  size_t look = cap * 8 < BZ_LOOK_MAX ? cap * 8 : BZ_LOOK_MAX; if (look < cap) look = cap;
  const size_t stage = look + BZ_MEMBER;
  size_t freeB = 0;
  s->resident = !s->oneWalk && mgFileStays (s->fileSize, &freeB);
  s->compCap = s->resident ? (size_t) s->fileSize : look + 2 * BZ_MEMBER;
  if (hipMalloc ((void **) &s->dStage[0], stage) != hipSuccess || hipMalloc ((void **) &s->dStage[1], stage) != hipSuccess
      || hipMalloc ((void **) &s->dComp, s->compCap) != hipSuccess)
    { mgHipFail (hipGetLastError (), "blocked gzip on the device"); s->release (); return -1; }
  const int rc = s->file.reserve (s->compCap, "blocked gzip on the device");
  if (rc || !s->edge.ready ()) { if (rc != -1) mgSetError ("blocked gzip %s: no page-locked memory", s->name.c_str ()); s->release (); return -1; }
  s->stageCap = stage; s->look = look; s->p = 0; s->at = s->have = 0; s->uploadedTo = 0;
  return 0;
}

/* the next members, as many as the staging buffer and the compressed bytes' buffer hold, inflated behind what the staging buffer has */
static int bzLoad (MgBgzfSrc *s, hipStream_t st)
{
  const U64 batchBytes = s->resident ? ~(U64) 0 : s->compCap;
  const size_t want = s->look;
  if (s->at)                                             /* the tail to the front of the other buffer */
    { if (s->have && hipMemcpyAsync (s->dStage[s->p ^ 1], s->dStage[s->p] + s->at, s->have, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return mgHipFail (hipGetLastError (), "blocked gzip on the device"), -1;
      s->p ^= 1; s->at = 0;
    }
  const size_t m0 = s->m; size_t e = m0, add = 0;
  const U64 a = s->start[m0];
  while (e < s->mem.size () && s->have + add < want && s->start[e + 1] - a <= batchBytes && e - m0 < ((size_t) 1 << 24))
    { add += s->mem[e].uLen; ++e; }
  const U64 b = s->start[e], base = s->resident ? 0 : a;
  { const U64 from = s->resident && s->uploadedTo > a ? s->uploadedTo : a;      /* (resident: what an earlier walk brought stays) */
    if (from < b)
      { const size_t n = (size_t) (b - from);
        const int rc = s->file.upload (s->fd, from, n, s->dComp + (from - base), st, "blocked gzip on the device");
        if (rc) { if (rc == -2) mgSetError ("failed to read sequence file %s", s->name.c_str ()); return -1; }
        mgInflateDiagUploaded (n);
        if (s->resident) s->uploadedTo = b;
      }
  }
  const U32 k = (U32) (e - m0);
  s->batch.resize (k); s->status.resize (k);
  size_t u = s->have;
  for (U32 i = 0 ; i < k ; ++i)
    { MgGzMember g = s->mem[m0 + i];
      g.cOff -= base; g.uOff = u; u += g.uLen;
      s->batch[i] = g;
    }
  const size_t workBytes = mgInflateWorkBytes (k);
  if (s->work.reserve (workBytes, workBytes + workBytes / 2 + 4096, "blocked gzip on the device")) return -1;
  U32 nBad = 0;
  if (mgInflateRun (s->dComp, s->resident ? s->fileSize : (U64) (b - a), s->batch.data (), k, s->dStage[s->p], s->stageCap, s->work.p, s->status.data (), &nBad, st) != MG_OK) return -1;
  if (nBad)
    for (U32 i = 0 ; i < k ; ++i)
      if (s->status[i])
        { mgSetError ("sequence file %s: corrupt blocked-gzip member at file offset %llu (inflate status %u)", s->name.c_str (), (unsigned long long) s->start[m0 + i], s->status[i]);
          return -1;
        }
  s->have += add; s->m = e;
  return 0;
}

extern "C" int mgBgzfSrcFill (MgBgzfSrc *s, unsigned char *dDst, size_t cap, U64 off, U64 limit, void *stream, size_t *n, int *more, U32 *first, U32 *last)
{
  hipStream_t st = (hipStream_t) stream;
  *n = 0; *more = 0; *first = *last = 0;
  const U64 end = limit < s->textBytes ? limit : s->textBytes;
  size_t want = 0;
  if (mgFillWant ("blocked gzip", s->name.c_str (), off, s->pos, end, cap, &want)) return -1;
  if (!want) return 0;
  if (bzReserve (s, cap)) return -1;
  while (s->have < want && s->m < s->mem.size ()) if (bzLoad (s, st)) { (void) hipStreamSynchronize (st); return -1; }
  const size_t take = s->have < want ? s->have : want;
  if (!take) return 0;
  const unsigned char *src = s->dStage[s->p] + s->at;
  if (hipMemcpyAsync (dDst, src, take, hipMemcpyDeviceToDevice, st) != hipSuccess) return mgHipFail (hipGetLastError (), "blocked gzip on the device"), -1;
  if (s->edge.fetch ("blocked gzip", src, take, st, first, last)) return -1;
  s->at += take; s->have -= take; s->pos += take;
  /* one walk: the empty members behind the text's last byte (bgzip's end marker) are part of the file -- uploaded and checked as every other */
  if (s->oneWalk && s->pos == s->textBytes)
    while (s->m < s->mem.size ()) if (bzLoad (s, st)) { (void) hipStreamSynchronize (st); return -1; }
  *n = take; *more = s->pos < end;
  return 0;
}
