/* mg_textsink.h — where the text of a walk goes (mg_seqconvert.hip, mg_filecodec.hip), the mirror of mg_textsrc.h: a FILE behind a writer thread, as it
 * is or as a blocked-gzip (BGZF) file deflated on the device (mg_bgzfsink.hip) */
#ifndef MG_TEXTSINK_H
#define MG_TEXTSINK_H
#include <condition_variable>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <time.h>
#include <unistd.h>
#include "mg_common.h"
#include "mg_internal.h"

/* The window of a walk that writes: a quarter of the parser's largest.  The output buffers are up to three windows each, two on the device and two page-locked,
   made per call; the kernels and the link do not gain from more than this */
#define TS_WINDOW_HINT ((size_t) 32 << 20)
static inline double tsMs (const struct timespec &a, const struct timespec &b) { return (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6; }

/* the windows' output, written in order behind the caller: two page-locked blocks, one being filled while the other is written */
struct TsWriter {
  FILE *out = 0;
  std::thread th; std::mutex mu; std::condition_variable cv;
  struct Block { unsigned char *p = 0; bool pinned = false; size_t n = 0; U64 spliceAt = 0, spliceCount = 0; int state = 0; } blk[2];      /* state: 0 free, 1 being filled, 2 to be written */
  U64 head = 0, tail = 0; bool closing = false, err = false, started = false;
  double msWrite = 0;
  int open (FILE *f, size_t cap)
  { out = f;
    for (int i = 0 ; i < 2 ; ++i)
      { blk[i].p = (unsigned char *) mgPinnedAlloc (cap); blk[i].pinned = blk[i].p != 0;
        if (!blk[i].p) blk[i].p = (unsigned char *) malloc (cap ? cap : 16);
        if (!blk[i].p) { mgSetError ("mgSeqConvert: out of memory"); return -1; }
      }
    try { th = std::thread (&TsWriter::run, this); started = true; } catch (...) { started = false; }      /* (no thread: every block is written on the spot) */
    return 0;
  }
  static bool bangs (FILE *f, U64 n)                     /* n times '!' */
  { char run[1 << 16];
    memset (run, '!', n < sizeof (run) ? (size_t) n : sizeof (run));
    while (n) { const size_t k = n < sizeof (run) ? (size_t) n : sizeof (run); if (fwrite (run, 1, k, f) != k) return false; n -= k; }
    return true;
  }
  void write (Block &b)                                  /* the block, with spliceCount times '!' behind its first spliceAt bytes (seqconvert's FASTA -> FASTQ) */
  { struct timespec t0, t1; clock_gettime (CLOCK_MONOTONIC, &t0);
    const size_t at = b.spliceCount ? (size_t) b.spliceAt : b.n;
    bool ok = fwrite (b.p, 1, at, out) == at;
    if (ok && b.spliceCount) ok = bangs (out, b.spliceCount) && fwrite (b.p + at, 1, b.n - at, out) == b.n - at;
    clock_gettime (CLOCK_MONOTONIC, &t1);
    msWrite += tsMs (t0, t1);
    if (!ok) err = true;
  }
  void run ()
  { std::unique_lock<std::mutex> lk (mu);
    for (;;)
      { Block &b = blk[head & 1];
        cv.wait (lk, [&] { return b.state == 2 || closing; });
        if (b.state != 2) return;
        lk.unlock (); write (b); lk.lock ();
        b.state = 0; ++head;
        cv.notify_all ();
      }
  }
  Block &acquire ()
  { std::unique_lock<std::mutex> lk (mu);
    Block &b = blk[tail & 1];
    cv.wait (lk, [&] { return b.state == 0; });
    b.state = 1;
    return b;
  }
  void submit (Block &b)
  { if (!started) { write (b); b.state = 0; ++tail; ++head; return; }
    std::lock_guard<std::mutex> lk (mu);
    b.state = 2; ++tail;
    cv.notify_all ();
  }
  int close ()
  { if (started) { { std::lock_guard<std::mutex> lk (mu); closing = true; cv.notify_all (); } th.join (); started = false; }
    for (int i = 0 ; i < 2 ; ++i) { if (blk[i].pinned) mgPinnedFree (blk[i].p); else free (blk[i].p); blk[i].p = 0; }
    return err ? -1 : 0;
  }
};

/* the BGZF sink's packed members: to a page-locked block of the writer thread's */
static int tsBgzfEmit (void *ctx, const unsigned char *src, size_t n, int onDevice, void *stream)
{
  TsWriter *wr = (TsWriter *) ctx;
  TsWriter::Block &b = wr->acquire ();
  int rc = 0;
  b.n = n; b.spliceAt = 0; b.spliceCount = 0;
  if (!onDevice) memcpy (b.p, src, n);
  else if (n && (hipMemcpyAsync (b.p, src, n, hipMemcpyDeviceToHost, (hipStream_t) stream) != hipSuccess || hipStreamSynchronize ((hipStream_t) stream) != hipSuccess))
    { b.n = 0; rc = -1; mgHipFail (hipGetLastError (), "blocked gzip on the device"); }
  wr->submit (b);
  return rc;
}

/* where the output goes: a FILE of the caller's, or a file that is opened once the text has been judged -- a refusal makes none.  The file is text, text
   through mgGzipOpenWrite (gz), or BGZF (bgzf): the sink that deflates on the device (device ()) and a writer thread of its own behind it */
struct TsSink {
  FILE *f = 0; const char *name = 0; bool gz = false, toStdout = false, opened = false, bgzf = false;
  TsWriter bzWr; MgBgzfSink *bz = 0; bool bzWrOpen = false; U64 textHint = 0;
  FILE *get ()
  { if (f || !name) return f;
    f = gz ? mgGzipOpenWrite (toStdout ? "/dev/stdout" : name) : toStdout ? fdopen (dup (1), "w") : fopen (name, "w");
    if (f) opened = true; else mgSetError ("failed to open output file %s", name);
    if (f && bgzf && (!(bz = mgBgzfSinkOpen (tsBgzfEmit, &bzWr, "mgSeqConvert", textHint)) || (bzWrOpen = true, bzWr.open (f, mgBgzfSinkEmitMax (bz))))) { (void) close (-1); return 0; }
    return f;
  }
  MgBgzfSink *device () { return bz; }
  int close (int rc)                                       /* the file is the call's: closed; none is left if the call failed (nor one from an earlier call: the program would have truncated it) */
  { if (bz && mgBgzfSinkClose (bz, !rc) && !rc) rc = -1;   /* (a call that failed leaves the BGZF file unfinished) */
    if (bzWrOpen && bzWr.close () && !rc) { mgSetError ("%s", "blocked gzip on the device: write failed"); rc = -1; }
    bz = 0; bzWrOpen = false;
    if (opened && fclose (f) && !rc) { mgSetError ("failed to write output file %s", name); rc = -1; }
    if (rc && name && !toStdout) (void) remove (name);
    if (opened) { f = 0; opened = false; }
    return rc;
  }
};
#endif
