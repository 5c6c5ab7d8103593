/* mg_textgpu.hip — the file front end on the device: plain FASTA text -> 2-bit packed reads, parsed by the GPU.
 *
 * What the reference's callers get from seqIOread for FASTA (seqio.c:302-323 with dna2indexConv after the N -> 0 patch,
 * modutils.c:39): a record starts at a '>' that is the first byte of a line, its header runs to the end of that line, its
 * sequence is every A/a C/c G/g T/t N/n (0 1 2 3 0) up to the next record start, all other bytes dropped.  The host parser
 * (mg_seqio.c) does that with a pool of threads at about 19 GB/s of text on the box's 16 allowed CPUs, which is what bounds
 * mgAddSequenceFile (12-14 Gbp/s file -> modset) under kernels that take 1 Tbp/s.  Here the host only moves bytes: the
 * file is read window by window straight into pinned memory (parallel pread: the copy out of the page cache), the window
 * goes across PCIe as it is, and three small kernels per window do the parsing:
 *
 *   "\n>" is a record start whatever came before (a header ends at its newline, so after a newline the state is always
 *   "sequence"); a byte lies in a header iff the LAST EVENT before it -- record start or newline -- is a record start.
 *   Events carry their position, so "last event" is a running maximum:
 *     K1  per tile of 4 KiB: the code (position << 1 | isStart) of its last event;
 *     K2  one workgroup: running maximum over the tiles (+ the state the previous window ended in) -> the state at every
 *         tile's first byte;
 *     K3  per tile: the bytes again, the running maximum inside the tile, per thread the bases and record starts of its
 *         16 bytes -> the tile's counts;
 *     K4  one workgroup: prefix sums of the counts, on top of what the batch holds already (device-resident totals);
 *     K5  per tile: the bytes a third time; bases (one byte each) and record offsets written where the sums say.
 *   The bases of complete records are packed to 2 bits (mgLaunchPack) and handed to mgAddReadsDevice a batch at a time; the
 *   record the batch ends in the middle of is carried to the front of the next batch on the device.
 *
 * FASTQ goes the same way with other kernels (see "FASTQ" in mg_textparse.hip): the line a byte belongs to is the number of newlines before
 * it, line mod 4 says what the byte is; the format's rules are checked on the device and never judged there.
 *
 * Return codes of the parser (txParseFile, mgAddSequenceFileDevice, mgTextForEachBatchDevice): 0 = the whole file; -1 = error
 * (mgLastError); -2 = not a file for this path -- ordinary gzip below MODGPU_GZIP_MIN_KB or under MODGPU_GZIP_HOST=1 (and whatever else mgBgzfSrcOpen
 * and mgGzipSrcOpen decline: blocked gzip followed by a foreign member, mg_pgzip.c's 16 MiB members, a truncated block), text whose last byte is not a newline (the reference reports
 * the unfinished record, seqio.c:213-217), FASTA text whose last line is a header, anything that is not a regular file, no
 * device, MODGPU_TEXT_HOST=1, blocked gzip under MODGPU_BGZF_HOST=1: the caller uses the host parser from the start; -3 = FASTQ text
 * that breaks a rule, or ends inside a record, somewhere after byte *resumeOff -- or FASTA text out of ordinary gzip whose last record, which
 * starts at byte *resumeOff, is unfinished: the records before it have been handed on, the host
 * parser continues from there (and says what the reference says).  mgTextParseFileDevice (the test hook) maps -3 to -2 and hands
 * nothing on.  Record ids (seqio.c:303-304) are extracted for the callers that print them (mgReferenceFastaRead, mgQueryFile), not for
 * mgAddSequenceFile (modutils.c:35 ignores them).
 *
 * A file that is blocked gzip (BGZF) from end to end is inflated on the device (mg_bgzfsrc.hip) straight into the window's device
 * buffer and parsed by the same loop; the windows come from one source with two makers (TxSrc, mg_text_int.h).  For such a file
 *   - the text size in the loop is the TEXT's size (mgBgzfSrcTextBytes), and what the parser looks at before it starts -- first byte,
 *     last byte, the last line -- comes from the first and the last members, inflated on the host (mgBgzfSrcEdges);
 *   - event codes, recPos / endP and *resumeOff carry TEXT offsets (the host parser is opened at a text offset: mg_seqio.c seqOpenAt);
 *   - prevByte comes from the source's `last` (no page-locked copy of the window exists), and the record ids from the id kernels
 *     ("record ids on the device", mg_textids.hip), not from the host team;
 *   - a member that does not inflate in the middle of the file is -1, the message naming the member's file offset.
 *
 * An ordinary gzip file of at least MODGPU_GZIP_MIN_KB is inflated on the device as well (mg_gzipsrc.hip over mg_gunzip.hip, one walk: the compressed
 * bytes pass through a bounded range) and parsed by the same loop through a third maker (txSrcGzip).  What differs from blocked gzip:
 *   - a deflate stream has no index, so only the text's first byte is known before the walk (the file's head inflated on the host); the size is a guess
 *     that sets the window, the text ends where the source says so, and FASTQ's verdict at the end works as it is;
 *   - the two FASTA cases a sized text is declined for up front -- no newline at the end, a header as the last line -- are met at the end, after
 *     records have been handed on: the records before the last one are handed on too, and the call returns -3 with the last record's '>' and its line
 *     number (1 + the newlines before it: counted window by window on the device, mgTextRecordLineKernel), where the host parser takes the file up
 *     (one host inflate up to that offset: mg_seqio.c seqOpenAt) and says what the reference says;
 *   - a corrupt stream in the middle of the file is -1 ("corrupt gzip stream at file offset N"), with what earlier windows handed on added.
 */
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include "mg_text_int.h"

/* of the calling thread's last file call (mgTextFileDiag): which parser took it (0 the host's from the start, 1 this one over plain text, 2 this one over
   blocked gzip inflated on the device, 3 this one over ordinary gzip inflated on the device), windows and text bytes parsed here, the text offset handed to the host parser */
thread_local U64 gTxDiag[4];
extern "C" void mgTextFileDiag (U64 out4[4]) { memcpy (out4, gTxDiag, sizeof (gTxDiag)); }

/* the file through the device parser; every batch of complete records goes to sink.  Returns 0, -1 (error: mgLastError), or -2
 * (not a file this path takes: the caller uses the host parser).  *nSeqOut / *totLenOut: records and bases of the file. */
static int txParseFile (const char *filename, const TxSink &sink, U64 *nSeqOut, U64 *totLenOut, U64 *resumeOff = 0, U64 *resumeLine = 0)
{
  memset (gTxDiag, 0, sizeof (gTxDiag)); mgInflateDiagReset (); mgGunzipDiagReset ();      /* the censuses are this call's */
  if (mgEnsureDevice ()) return -2;
  if (mgKnobs ()->textHost == 1) return -2;      /* test knob: the host parser */
  struct Input { int fd = -1; MgBgzfSrc *bz = 0; MgGzipSrc *gz = 0; ~Input () { if (bz) mgBgzfSrcClose (bz); if (gz) mgGzipSrcClose (gz); if (fd >= 0) close (fd); } } in;      /* closed on whichever return */
  in.fd = open (filename, O_RDONLY);
  if (in.fd < 0) return -2;
  const int fd = in.fd;
  struct stat sb;
  if (fstat (fd, &sb) || !S_ISREG (sb.st_mode) || sb.st_size < 2) return -2;
  /* what is looked at before anything starts: the text's size, its first byte, its last bytes (4096, or all of it) -- preads of a plain file, the
     first and the last members of blocked gzip inflated on the host.  Ordinary gzip has no index: the first byte comes from the file's head inflated on
     the host, the size is a guess, and the loop settles the text's end when it gets there (txParseText, sized = false) */
  size_t fileSize = (size_t) sb.st_size;
  unsigned char first = 0, magic[2] = { 0, 0 }, tail[4096]; size_t tn = 0;
  if (pread (fd, magic, 2, 0) != 2) return -2;
  if (magic[0] == 0x1f && magic[1] == 0x8b)
    { /* blocked gzip from end to end (MODGPU_BGZF_HOST=1, a test knob: inflated on the host, as on every other path); else ordinary gzip of a size the
         device takes (mgGzipSrcOpen: MODGPU_GZIP_MIN_KB, MODGPU_GZIP_HOST=1); else -- a 'BC' member followed by a foreign one, mg_pgzip.c's 16 MiB
         members, a truncated block, a small file -- the host reader's */
      if (mgKnobs ()->bgzfHost != 1 && !mgBgzfSrcOpen (filename, fd, (U64) sb.st_size, &in.bz))
        { mgBgzfSrcOneWalk (in.bz);                       /* (the compressed file does not stay on the device: that memory is the modset table's) */
          fileSize = (size_t) mgBgzfSrcTextBytes (in.bz);
          if (fileSize < 2 || mgBgzfSrcEdges (in.bz, &first, tail, sizeof (tail), &tn)) return -2;      /* (a member that does not inflate: the host parser reports it) */
        }
      else
        { if (mgGzipSrcOpen (filename, fd, (U64) sb.st_size, MG_GZIP_ONE_WALK, &in.gz)) return -2;      /* (one walk, for the same reason) */
          const int f = mgGzipSrcFirstByte (in.gz);
          if (f != '>' && f != '@') return -2;            /* (nothing has been handed on) */
          first = (unsigned char) f;
          fileSize = (size_t) mgGzipSrcSizeHint (in.gz);
        }
    }
  else
    { tn = fileSize < sizeof (tail) ? fileSize : sizeof (tail);
      first = magic[0];
      if (pread (fd, tail, tn, (off_t) (fileSize - tn)) != (ssize_t) tn) return -2;
    }
  if (!in.gz)
    { if ((first != '>' && first != '@') || tail[tn - 1] != '\n') return -2;
      if (first == '>')                                   /* FASTA text whose LAST line is a header: the reference reports the record as incomplete and does not
                                                             return it (seqio.c:213-217,314) -- left to the host parser, which says so with the line number */
        { size_t i = tn - 1;                               /* the final newline */
          while (i > 0 && tail[i - 1] != '\n') --i;        /* start of the last line (or of the tail: a header longer than that is no record id line we want to judge here) */
          if (tail[i] == '>' && (i > 0 || tn == fileSize)) return -2;
        }
    }

  int curDev = 0;
  if (hipGetDevice (&curDev) != hipSuccess || curDev < 0 || curDev >= TX_MAXDEV) { (void) hipGetLastError (); return -2; }      /* (no room kept for that device: the host parser) */
  TxBufs &t = gTxs[curDev];
  std::lock_guard<std::mutex> g (t.lock);
  TxPlain plain; plain.fd = fd; plain.size = fileSize; plain.nThreads = txHostThreads ();
  TxBgzf bgzf; bgzf.bz = in.bz; bgzf.size = fileSize;
  TxGzip gzip; gzip.gz = in.gz;
  const TxSrc src = in.bz ? txSrcBgzf (&bgzf) : in.gz ? txSrcGzip (&gzip) : txSrcPlain (&plain);
  const bool devIds = in.bz || in.gz || mgKnobs ()->textIdsDevice == 1;      /* a device source has no page-locked window for the host team */
  gTxDiag[0] = in.bz ? 2 : in.gz ? 3 : 1;
  return txParseText (first == '@', src, fileSize, !in.gz, devIds, t, sink, nSeqOut, totLenOut, resumeOff, resumeLine);
}

/* ---- sinks ---- */

struct TxAddCtx { Modset *ms; U64 totHash; };
static int txAddSink (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *, const U64 *, hipStream_t st)
{
  TxAddCtx *c = (TxAddCtx *) v;
  U64 nHash = 0;
  if (mgAddReadsDevice (c->ms, dPacked, total, dOff, nReads, &nHash, (void *) st) != MG_OK) return -1;
  c->totHash += nHash;
  return 0;
}

/* modutils.c:33-51 with the text parsed on the device.  0: done (counts filled in); -1: error; -2: not a file for this path */
extern "C" int mgAddSequenceFileDevice (Modset *ms, const char *filename, U64 *nSeq, U64 *totLen, U64 *totHash, U64 *resumeOff, U64 *resumeLine)
{
  TxAddCtx c; c.ms = ms; c.totHash = 0;
  TxSink sink; sink.fn = txAddSink; sink.ctx = &c; sink.wantIds = false;
  const int rc = txParseFile (filename, sink, nSeq, totLen, resumeOff, resumeLine);
  if (totHash) *totHash = c.totHash;
  return rc;
}

/* the sink of a 10x file (modutils.c:44): a batch holds complete records only -- the FASTA path carries the open record to the front of
   the next batch, the FASTQ path the bases of the open line -- so the records handed on so far say which of this batch's are the odd
   ones.  The batch is trimmed into the sink's own arrays (mgTrim10xDevice, mg_modutils.hip) and added from there */
struct TxAdd10xCtx { Modset *ms; U64 totHash, recsDone; MgDevBuf<U32> dPacked; MgDevBuf<U64> dOff; };
static int txAdd10xSink (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *, const U64 *, hipStream_t st)
{
  TxAdd10xCtx *c = (TxAdd10xCtx *) v;
  const size_t nw = mgPackedWords (total);
  if (c->dPacked.reserve (nw, nw + nw / 8, "10x trim") || c->dOff.reserve ((size_t) nReads + 1, ((size_t) nReads + 1) * 2, "10x trim")) return -1;
  U64 outBases = 0, nHash = 0;
  if (mgTrim10xDevice (dPacked, total, dOff, nReads, c->recsDone + 1, c->dPacked.p, c->dOff.p, &outBases, (void *) st) != MG_OK) return -1;
  mgAdd10xDiagBatch (nReads, c->recsDone + 1, total - outBases);
  if (mgAddReadsDevice (c->ms, c->dPacked.p, outBases, c->dOff.p, nReads, &nHash, (void *) st) != MG_OK) return -1;
  if (hipStreamSynchronize (st) != hipSuccess) return -1;            /* (the next batch's trim writes the same arrays) */
  c->totHash += nHash; c->recsDone += nReads;
  return 0;
}

extern "C" int mgAddSequenceFile10xDevice (Modset *ms, const char *filename, U64 *nSeq, U64 *totLen, U64 *totHash, U64 *resumeOff, U64 *resumeLine)
{
  TxAdd10xCtx c; c.ms = ms; c.totHash = 0; c.recsDone = 0;
  TxSink sink; sink.fn = txAdd10xSink; sink.ctx = &c; sink.wantIds = false;
  const int rc = txParseFile (filename, sink, nSeq, totLen, resumeOff, resumeLine);
  c.dPacked.drop (); c.dOff.drop ();
  if (totHash) *totHash = c.totHash;
  return rc;
}

/* modmap's file entry points (mgReferenceFastaRead, mgQueryFile: modmap.c:93-134,188-281): every batch of complete records,
   device resident, with the records' ids, to a C callback.  0 / -1 / -2 / -3 as txParseFile */
struct TxCbCtx { MgTextBatchFn fn; void *ctx; };
static int txCbSink (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, hipStream_t st)
{ TxCbCtx *c = (TxCbCtx *) v; return c->fn (c->ctx, dPacked, total, dOff, nReads, idBytes, idOff, (void *) st); }
extern "C" int mgTextForEachBatchDevice (const char *filename, MgTextBatchFn fn, void *ctx, U64 batchBases, U64 batchRecs, U64 *nSeq, U64 *totLen, U64 *resumeOff, U64 *resumeLine)
{
  TxCbCtx c; c.fn = fn; c.ctx = ctx;
  TxSink sink; sink.fn = txCbSink; sink.ctx = &c; sink.wantIds = true; sink.batchBases = batchBases; sink.batchRecs = batchRecs;
  return txParseFile (filename, sink, nSeq, totLen, resumeOff, resumeLine);
}

/* test hook: the device parser's records as host arrays (bases 0..3 one per byte, offsets[nSeq + 1]), malloc()ed */
struct TxHostCtx { std::vector<unsigned char> bases; std::vector<int64_t> offs; };
static int txHostSink (void *v, const U32 *dPacked, U64 total, const U64 *dOff, U32 nReads, const char *idBytes, const U64 *idOff, hipStream_t st)
{
  TxHostCtx *c = (TxHostCtx *) v;
  std::vector<U64> o ((size_t) nReads + 1);
  if (hipMemcpy (o.data (), dOff, ((size_t) nReads + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  MgDevScratch scratch ("mgTextParseFileDevice");
  unsigned char *dB;
  if (scratch.get (&dB, total ? total : 16)) return -1;
  if (mgLaunchUnpack (dPacked, total, dB, st) != MG_OK || hipStreamSynchronize (st) != hipSuccess) return -1;
  const size_t at = c->bases.size ();
  c->bases.resize (at + total);
  if (total && hipMemcpy (c->bases.data () + at, dB, total, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (c->offs.empty ()) c->offs.push_back (0);
  for (U32 r = 1 ; r <= nReads ; ++r) c->offs.push_back ((int64_t) (at + o[r]));
  return 0;
}
extern "C" int mgTextParseFileDevice (const char *filename, char **basesOut, int64_t **offsetsOut, int64_t *nSeqOut)
{
  TxHostCtx c;
  TxSink sink; sink.fn = txHostSink; sink.ctx = &c; sink.wantIds = false;
  U64 nSeq = 0, totLen = 0;
  const int rc = txParseFile (filename, sink, &nSeq, &totLen);
  if (rc) return rc == -3 ? -2 : rc;                       /* (FASTQ handed back to the host parser in the middle: nothing of it is returned here) */
  if (c.offs.empty ()) c.offs.push_back (0);
  char *b = (char *) malloc (c.bases.size () + 1); int64_t *o = (int64_t *) malloc (c.offs.size () * sizeof (int64_t));
  if (!b || !o) { free (b); free (o); return -1; }
  memcpy (b, c.bases.data (), c.bases.size ()); memcpy (o, c.offs.data (), c.offs.size () * sizeof (int64_t));
  *basesOut = b; *offsetsOut = o; *nSeqOut = (int64_t) nSeq;
  return 0;
}
