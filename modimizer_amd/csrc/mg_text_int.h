/* mg_text_int.h — what the files of the device text parser share (C++ only; mg_textgpu.hip, mg_textwin.hip, mg_textparse.hip, mg_textids.hip):
 * the per-device buffers and their owners, the window source and the window walk, the record ids, the sink.
 * mg_textgpu.hip's file comment says what the parser does and what it returns. */
#ifndef MG_TEXT_INT_H
#define MG_TEXT_INT_H
#include <mutex>
#include <vector>
#include "mg_prefix.h"
#include "mg_internal.h"

#define TX_PER   16                                      /* bytes per thread: one 16-byte load */
#define TX_TILE  MG_TEXT_TILE                            /* 4 KiB of text per workgroup of 256 threads (the kernels' files name the thread count) */

struct TxState {                                         /* FASTA, device resident, carried from window to window */
  U64 lastEvent;        /* code of the last event of the text so far: bit 0 = it was a record start (we are in a header) */
  U64 accBases;         /* bases in the batch accumulator */
  U64 accRecs;          /* record starts in the batch accumulator */
};
struct TqState {                                         /* FASTQ */
  U64 nlCount;          /* newlines of the file so far */
  U64 accBases, accQual, accRecs;      /* of the batch accumulator: bases, quality bytes, completed records */
  U64 bad;              /* != 0: a rule was broken somewhere in the accumulator's text */
};

static inline bool txTiming (void) { return mgKnobs ()->textTiming == 1; }   /* dev knob */
struct TxClock { double reserve = 0, read = 0, wait = 0, flush = 0, ids = 0, sink = 0, t0 = 0; void lap (double &slot) { const double n = mgNowS (); slot += n - t0; t0 = n; } };

/* ---- owners.  MgDevBuf (mg_common.h) for device arrays whose contents need not survive a growth; the two below for the rest ---- */
/* page-locked host memory (mgPinnedAlloc) that only grows, by a quarter more than asked; what it held is not kept */
template <class T> struct TxPinned {
  T *p = 0; size_t cap = 0;
  bool reserve (size_t want)
  { if (cap >= want) return true;
    drop ();
    if (!(p = (T *) mgPinnedAlloc ((want + want / 4) * sizeof (T)))) return false;
    cap = want + want / 4; return true;
  }
  void drop () { mgPinnedFree (p); p = 0; cap = 0; }
};
/* a device array that grows to cap elements and keeps its first `keep` (the batch accumulator: the capacity is its owner's, several arrays share one) */
template <class T> struct TxKeep {
  T *p = 0;
  bool grow (size_t keep, size_t cap)
  { T *n = 0;
    if (hipMalloc ((void **) &n, cap * sizeof (T)) != hipSuccess) return false;
    if (p) { (void) hipMemcpy (n, p, keep * sizeof (T), hipMemcpyDeviceToDevice); (void) hipFree (p); }
    p = n; return true;
  }
  void drop () { if (p) (void) hipFree (p); p = 0; }
};

/* ---- the buffers of one device (mg_textwin.hip): kept between calls, a call holds `lock` ---- */
struct TxBufs {
  int dev = -1;
  size_t window = 0;
  unsigned char *hPin[2] = { 0, 0 }, *dText[2] = { 0, 0 }; hipEvent_t h2dDone[2] = { 0, 0 };      /* a window page-locked and on the device, twice; its copy is over */
  hipStream_t copy = 0;
  U64 *hCounts = 0;                    /* pinned: what K4 / Kq4 leave for the host; word 6: the id kernels' total */
  MgDevBuf<TxState> dState; MgDevBuf<TqState> dTq; MgDevBuf<U32> dOverflow;
  MgDevBuf<U64> dOpenLine;             /* FASTA from a source of unknown size: the line number of the last record start so far (mgTextRecordLineKernel) */
  MgDevBuf<U64> dTileEvent, dTileBaseOff, dTileStartOff, dTileOffQ; MgDevBuf<U32> dTileBases, dTileStarts, dTileQual;      /* per tile (dTileOffQ, dTileQual: FASTQ's third counted quantity) */
  TxKeep<unsigned char> dBases; size_t basesCap = 0;      /* the batch accumulator: one byte a base ... */
  TxKeep<U64> dRecOff, dEndQ, dEndP, dRecPos; size_t recCap = 0;      /* ... and per record: its offset; FASTQ: quality bytes and text position at its end; FASTA: the text position of its '>' */
  MgDevBuf<U32> dPacked;
  TxPinned<U64> hHdr;                  /* where a window's record headers start (4e5 of them in a window of short reads: into pageable memory the copy took as long as extracting the ids) */
  MgDevBuf<U32> dIdLen, dIdLenT, dIdPlace; MgDevBuf<unsigned char> dIdBytes;      /* the id kernels: per header its id's length, that + 1 if it ends in the window, its place; the ids' bytes */
  TxPinned<unsigned char> hIdBytes; TxPinned<U32> hIdPlace;      /* ... and where they land */
  std::mutex lock;
  void release ();
};
#define TX_MAXDEV 128
extern TxBufs gTxs[TX_MAXDEV];                       /* by device: a process whose host threads read a file each on a GPU each parses them side by side */
/* buffers for windows of `window` bytes on the current device, the accumulator with room for basesNeed bases and recsNeed records (what it holds is
   kept).  0, or -1 with everything given back */
int txReserve (TxBufs &t, size_t window, U64 basesNeed, U64 recsNeed);
int txHostThreads (void);
size_t txWindowBytes (size_t fileSize);
U64 txBatchBases (U64 asked);

/* ---- where a window's text comes from: ONE loader for the parser and for the window streamer ----
 * A host source (fill) fills the page-locked buffer and the copy to the device is started; a device source (dfill) fills the device buffer itself by
 * work on the copy stream.  Either way h2dDone[i] is recorded behind it.  Three makers for the parser: the plain file (its team of readers), a
 * blocked-gzip file inflated on the device (mg_bgzfsrc.hip), and an ordinary gzip file inflated there (mg_gzipsrc.hip), whose text has no known size:
 * its fill is asked for windows until one says that no text follows. */
struct TxSrc { MgTextFillFn fill = 0; MgTextDevFillFn dfill = 0; void *src = 0; };
struct TxGot { size_t n = 0; int more = 0; U32 first = 0, last = 0; };   /* the window's bytes, whether text follows, its first and last byte */
struct TxPlain { int fd; U64 size; int nThreads; };
struct TxBgzf { MgBgzfSrc *bz; U64 size; };              /* size: the text's */
struct TxGzip { MgGzipSrc *gz; };
TxSrc txSrcPlain (TxPlain *p);
TxSrc txSrcBgzf (TxBgzf *b);
TxSrc txSrcGzip (TxGzip *z);

/* ---- the window walk: the alternation of the two buffers and nothing else.  Every step 0, -1 (the error is set) or -2 (HIP) ----
 *   start ();  while (got.n) { awaitCopy (); <kernels over dText ()>; loadNext (); <synchronise st, the rest of the window>; advance (); }
 * The window's copy was started as soon as it was read (copy stream); the next one is read into the other page-locked buffer and goes across the
 * link -- or is inflated into the other device buffer -- beside this window's kernels. */
struct TxWalk {
  TxBufs &t; const TxSrc &src; const size_t window; const hipStream_t st; TxClock *const ck;      /* ck != 0: its flush and read slots are lapped around every load */
  TxGot got, nxt;                      /* the current window; after loadNext (): the one behind it (n == 0: none) */
  U64 off = 0, index = 0;              /* the current window's first byte in the text; its number */
  U32 prevByte = '\n';                 /* the byte before the current window (a newline before the text's first byte) */
  bool eof = false;                    /* after loadNext (): the current window is the text's last */
  TxWalk (TxBufs &t_, const TxSrc &src_, size_t window_, hipStream_t st_, TxClock *ck_ = 0) : t (t_), src (src_), window (window_), st (st_), ck (ck_) {}
  int cur () const { return (int) (index & 1); }
  const unsigned char *dText () const { return t.dText[cur ()]; }
  const unsigned char *hText () const { return src.dfill ? 0 : t.hPin[cur ()]; }      /* 0: a device source has no page-locked copy of the window */
  int start ();                        /* window 0 is on its way */
  int awaitCopy ();                    /* st waits for the current window's copy */
  int loadNext ();                     /* the window behind the current one, into the other buffer once that one's last copy is over */
  void advance ();
  void drain ();                       /* after a failure: nothing of this call is left in flight over buffers the next one takes */
private:
  int load (int i, U64 at, TxGot *o);
};

/* ---- record ids (mg_textids.hip; seqio.c:303-304: the header line after its '>' / '@' up to the first white space) ----
 * The ids of the accumulator's records, in record order.  The kernels say where every header starts (FASTA: mgTextEmitKernel's recPos; FASTQ: the
 * byte after a record's last newline, endP + 1); the few bytes up to the first white space are copied out of the page-locked window by a team of
 * host threads, or cut out on the device by the id kernels.  An id that runs on into the next window (or starts at its first byte) is finished when
 * that window is in. */
struct TxIds {
  std::vector<char> bytes; std::vector<U64> off;           /* id r = bytes + off[r], 0-terminated */
  std::vector<U64> hdr;                                    /* (a window's header positions, for the host team) */
  bool open = false; bool skipOne = false;                 /* the last id is not finished; its '@' is the next window's first byte */
  double tLens = 0, tDev = 0;       /* (dev timing: the host team's two passes, the id kernels with their copies) */
  static inline bool space (unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }      /* isspace in the C locale (not isspace (): that one follows the process's locale; seqio.c:303) */
  void feed (const unsigned char *p, size_t n);
  void header (const unsigned char *win, size_t n, size_t at);
  void headersTeam (const unsigned char *win, size_t n, const U64 *at, size_t cnt, int nThreads);
  void headers (const unsigned char *win, size_t n, std::vector<U64> &at, int nThreads);
  void dropFront (size_t nRec);                            /* the first nRec records were flushed */
};
/* the headers that start in the current window: dSrc[0 .. n) + add are their ids' first bytes as text offsets; at0: one more at the window's byte 0 */
struct TxHdrs { const U64 *dSrc = 0; U64 add = 0; size_t n = 0; bool at0 = false; };
/* behind the emit kernel: st is waited for -- with the header positions in t.hHdr where the host team will want them (toHost) */
int txHeadersOut (TxBufs &t, bool toHost, const TxHdrs &h, hipStream_t st);
/* the ids of the current window appended to ids, by the id kernels (devIds) or by the host team after txHeadersOut.  0 / -1 */
int txWindowIds (TxBufs &t, TxIds &ids, bool devIds, const TxWalk &wk, const TxHdrs &h, int nThreads, hipStream_t st);

/* ---- the parse loop (mg_textparse.hip) and what it hands a batch of complete records to ---- */
struct TxSink {
  int (*fn) (void *ctx, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, U32 nReads, const char *idBytes, const U64 *idOff, hipStream_t st);
  void *ctx;
  U64 batchBases = 0;                                      /* != 0: a batch is handed on once it holds this many bases (the knobs, which tests set, come first) */
  U64 batchRecs = 0;                                       /* != 0: ... and this many records -- or the default batch's bases whatever the records (long reads: few lines to format, and a batch's chaining costs its LONGEST read's serial walk: fewer, larger batches) */
  bool wantIds;                                            /* id r = idBytes + idOff[r], 0-terminated */
};
/* the text of `src` (FASTQ or FASTA) through the kernels, every batch of complete records to sink.  textSize: the text's size, which sets the window;
   sized = false: a guess, the text ends where the source says so, and what the callers of a sized text look at before they start -- the last byte, the
   last line -- is settled at the end.  0 = the whole text; -1 = error; -3 = the text from byte *resumeOff on (a record start, line *resumeLine) is left
   to the host parser, the records before it have been handed on: FASTQ, a rule of the format is broken somewhere after it, or the text ends in the
   middle of a record; FASTA of unknown size, the text's last byte is no newline or its last line is a header, and the record is the last one -- the
   host parser then reports what the reference reports (seqio.c:213-217,314,326-339) */
int txParseText (bool fastq, const TxSrc &src, size_t textSize, bool sized, bool devIds, TxBufs &t, const TxSink &sink, U64 *nSeqOut, U64 *totLenOut, U64 *resumeOff, U64 *resumeLine);
extern thread_local U64 gTxDiag[4];                      /* mg_textgpu.hip (mgTextFileDiag) */
#endif
