/* mg_devfile.h — what the readers of a whole file on the device share (mg_bgzfsrc.hip, mg_gzipsrc.hip, mg_filecodec.hip): the file's bytes to the device in
 * page-locked pieces, the rule by which a compressed file stays there, and the head and the tail of a source's fill (the MgTextDevFillFn contract) */
#ifndef MG_DEVFILE_H
#define MG_DEVFILE_H
#include <string>
#include "mg_common.h"
#include "mg_knobs.h"
#include "mg_internal.h"

/* bytes per read and upload: 16 MiB (MODGPU_FILE_PIECE_KB: dev, 4 KiB at least, so that a test's file of a few KiB crosses pieces) */
static inline size_t mgFilePieceBytes (void)
{ const long v = mgKnobs ()->filePieceKb; return (size_t) (v == MG_KNOB_UNSET ? 16384 : v < 4 ? 4 : v > (1 << 20) ? (1 << 20) : v) << 10; }
/* a compressed file stays on the device up to 8 GiB, and only in a quarter of the free memory (*freeB; 0 if the runtime does not say) */
#define MG_FILE_RESIDENT_MAX ((U64) 8 << 30)
static inline bool mgFileStays (U64 fileSize, size_t *freeB) { *freeB = 0; return fileSize <= MG_FILE_RESIDENT_MAX && mgDevFreeBytes (freeB) && fileSize <= *freeB / 4; }

/* A file's bytes to the device: two page-locked pieces, one is read by the parser's team of readers (mgTextReadParallel) while the one before it is on the link.
   The count of pieces runs on from call to call, so that a piece an earlier call left on the link is waited for before its memory is read into again.
   Both calls: 0, -1 = a HIP call failed (reported as `what`), -2 = no page-locked memory / the read failed (the message is the caller's, who names the file) */
struct MgDevFile {
  unsigned char *h[2] = { 0, 0 }; hipEvent_t up[2] = { 0, 0 }; size_t piece = 0; U64 pieces = 0;
  int reserve (size_t most, const char *what)            /* pieces for uploads of at most `most` bytes a call */
  { release ();
    piece = most < mgFilePieceBytes () ? most : mgFilePieceBytes ();
    for (int i = 0 ; i < 2 && piece ; ++i)
      { if (hipEventCreateWithFlags (&up[i], hipEventDisableTiming) != hipSuccess) { up[i] = 0; mgHipFail (hipGetLastError (), what); release (); return -1; }
        if (!(h[i] = (unsigned char *) mgPinnedAlloc (piece))) { release (); return -2; }
      }
    return 0;
  }
  int upload (int fd, U64 fileOff, size_t n, unsigned char *dDst, hipStream_t st, const char *what)      /* [fileOff, fileOff + n) of fd to dDst by copies on st; the last of them may still be on the link */
  { for (size_t done = 0 ; done < n ; done += piece, ++pieces)
      { const int k = (int) (pieces & 1);
        const size_t part = n - done < piece ? n - done : piece;
        if (pieces >= 2 && hipEventSynchronize (up[k]) != hipSuccess) return mgHipFail (hipGetLastError (), what), -1;
        if (mgTextReadParallel (fd, h[k], part, (int64_t) (fileOff + done))) return -2;
        if (hipMemcpyAsync (dDst + done, h[k], part, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord (up[k], st) != hipSuccess) return mgHipFail (hipGetLastError (), what), -1;
      }
    return 0;
  }
  void release ()
  { for (int i = 0 ; i < 2 ; ++i) { mgPinnedFree (h[i]); h[i] = 0; if (up[i]) (void) hipEventDestroy (up[i]); up[i] = 0; }
    piece = 0; pieces = 0;
  }
};

/* The head of a fill: the source stands at byte `pos` of its text and is asked for the bytes from `off` on, below `end`, into a window of cap bytes.
   -1 = off is not pos ("<kind> <name>: byte .. asked for at byte .."), else 0 and *want: the bytes the window takes, 0 = none */
static inline int mgFillWant (const char *kind, const char *name, U64 off, U64 pos, U64 end, size_t cap, size_t *want)
{
  if (off != pos) { mgSetError ("%s %s: byte %llu asked for at byte %llu", kind, name, (unsigned long long) off, (unsigned long long) pos); return -1; }
  *want = off >= end ? 0 : end - off < cap ? (size_t) (end - off) : cap;
  return 0;
}
/* The tail of a fill: the first and the last of the n > 0 device bytes at d into *first and *last, behind the fill's work on st, which is over when it returns.
   The two bytes cross into a page-locked block of the fill's own, made (ready ()) before the fill queues any work.  0, -1 with the error set ("<kind> on the device") */
struct MgFillEdge {
  unsigned char *h = 0;
  bool ready () { return h || (h = (unsigned char *) mgPinnedAlloc (64)); }
  int fetch (const char *kind, const unsigned char *d, size_t n, hipStream_t st, U32 *first, U32 *last)
  { if (hipMemcpyAsync (h, d, 1, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync (h + 1, d + n - 1, 1, hipMemcpyDeviceToHost, st) != hipSuccess
        || hipStreamSynchronize (st) != hipSuccess) return mgHipFail (hipGetLastError (), (std::string (kind) + " on the device").c_str ()), -1;
    *first = h[0]; *last = h[1];
    return 0;
  }
  void release () { mgPinnedFree (h); h = 0; }
};
#endif
