/* mg_filecodec.hip — `bgzip -d`, `gzip -dc` and `bgzip` as calls: a compressed file's text inflated on the device (mg_bgzfsrc.hip, mg_gzipsrc.hip), and any
 * regular file deflated there as BGZF (mg_bgzfsink.hip).  The file's bytes cross in page-locked pieces (mg_devfile.h); what comes back goes to the writer
 * thread of mg_textsink.h.  Nothing here looks at the text */
#include <fcntl.h>
#include <sys/stat.h>
#include "mg_devfile.h"
#include "mg_textsrc.h"
#include "mg_textsink.h"

/* inName open for reading and *size, if it is a regular file: the descriptor, -1 = it does not open (the error is set), -2 = not a regular file (nothing stays open, no error is set) */
static int fcOpen (const char *inName, U64 *size)
{
  struct stat sb;
  const int fd = ::open (inName, O_RDONLY);
  if (fd < 0) { mgSetError ("failed to open file %s", inName); return -1; }
  if (fstat (fd, &sb) || !S_ISREG (sb.st_mode)) { ::close (fd); return -2; }
  *size = (U64) sb.st_size;
  return fd;
}

/* mgBgzfInflateFile and mgGzipInflateFile: they differ in the source that is opened.  Its text goes window by window to the writer thread: window k + 1 is
   inflated while window k crosses to a page-locked block and the block before that is written.  0, -2 = not such a file (nothing is written), -1 */
static int fcInflateFile (const char *what, const char *inName, const char *outName, bool bgzf)
{
  mgInflateDiagReset (); if (!bgzf) mgGunzipDiagReset ();
  if (!inName || !outName) { mgSetError ("%s: no file name", what); return -1; }
  CpSource src; src.name = inName;
  U64 size = 0;
  if ((src.fd = fcOpen (inName, &size)) < 0) return src.fd;
  int rc = !size ? -2 : bgzf ? mgBgzfSrcOpen (inName, src.fd, size, &src.bz) : mgGzipSrcOpen (inName, src.fd, size, 1, &src.gz);
  if (rc) { src.close (); return rc; }
  const U64 textHint = bgzf ? mgBgzfSrcTextBytes (src.bz) : mgGzipSrcSizeHint (src.gz);
  TsSink sink; sink.name = outName; sink.toStdout = !strcmp (outName, "-");
  const size_t window = mgTextWindowBytes ((size_t) (textHint < TS_WINDOW_HINT ? textHint : TS_WINDOW_HINT));
  MgDevScratch scratch (what);
  unsigned char *dBuf[2] = { 0, 0 };
  hipStream_t inflate = 0, copy = 0;
  TsWriter wr; bool wrOpen = false;
  FILE *out = 0;
  TsWriter::Block *pending = 0;                          /* the block a window is crossing into */
  bool bad = false;
  auto land = [&] () { if (!pending) return; if (hipStreamSynchronize (copy) != hipSuccess) { scratch.fail (); bad = true; pending->n = 0; } wr.submit (*pending); pending = 0; };
  rc = -1;
  do
    { if (mgEnsureDevice ()) break;
      if (scratch.get (&dBuf[0], window) || scratch.get (&dBuf[1], window)) break;
      if (hipStreamCreateWithFlags (&inflate, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags (&copy, hipStreamNonBlocking) != hipSuccess) { scratch.fail (); break; }
      if (!(out = sink.get ())) break;
      wrOpen = true;
      if (wr.open (out, window)) break;
      U64 off = 0; int more = 1;
      for (U64 k = 0 ; more && !bad ; ++k)
        { size_t n = 0; U32 first, last;
          if (CpSource::dfill (&src, dBuf[k & 1], window, off, (void *) inflate, &n, &more, &first, &last)) { bad = true; break; }
          land ();
          if (bad || !n) break;
          TsWriter::Block &b = wr.acquire ();
          b.n = n; b.spliceAt = 0; b.spliceCount = 0;
          if (hipMemcpyAsync (b.p, dBuf[k & 1], n, hipMemcpyDeviceToHost, copy) != hipSuccess) { scratch.fail (); b.n = 0; wr.submit (b); bad = true; break; }
          pending = &b; off += n;
        }
      land ();
      if (!bad) rc = 0;
    }
  while (0);
  if (wrOpen && wr.close () && !rc) { mgSetError ("%s: write failed", what); rc = -1; }
  if (inflate) { (void) hipStreamSynchronize (inflate); (void) hipStreamDestroy (inflate); }
  if (copy) { (void) hipStreamSynchronize (copy); (void) hipStreamDestroy (copy); }
  rc = sink.close (rc);
  src.close ();
  return rc;
}
extern "C" int mgBgzfInflateFile (const char *inName, const char *outName, FILE *err) { (void) err; return fcInflateFile ("mgBgzfInflateFile", inName, outName, true); }
/* `gzip -dc`: 0, -2 = not ordinary gzip (or more than the device keeps; nothing is written), -1 with mgLastError () and no output file left.  Any size is taken */
extern "C" int mgGzipInflateFile (const char *inName, const char *outName, FILE *err) { (void) err; return fcInflateFile ("mgGzipInflateFile", inName, outName, false); }

/* `bgzip`: any regular file as BGZF.  A piece of the file crosses the link as it is and the sink (mg_bgzfsink.hip) deflates it on the device, which has the
   piece by then: the next one is read when the sink is done with this one.  Only the compressed file comes back, to the sink's writer thread */
extern "C" int mgBgzfDeflateFile (const char *inName, const char *outName, FILE *err)
{
  (void) err;
  mgDeflateDiagReset ();
  if (!inName || !outName) { mgSetError ("mgBgzfDeflateFile: no file name"); return -1; }
  U64 size = 0;
  const int fd = fcOpen (inName, &size);
  if (fd == -2) mgSetError ("mgBgzfDeflateFile: %s is not a regular file", inName);
  if (fd < 0) return -1;
  TsSink sink; sink.name = outName; sink.toStdout = !strcmp (outName, "-"); sink.bgzf = true; sink.textHint = size ? size : 1;
  MgDevScratch scratch ("mgBgzfDeflateFile");
  MgDevFile file;
  unsigned char *dPiece = 0;
  int rc = mgEnsureDevice () ? -1 : file.reserve ((size_t) size, "mgBgzfDeflateFile");
  if (rc == -2) mgSetError ("mgBgzfDeflateFile: no page-locked memory");
  if (!rc && ((file.piece && scratch.get (&dPiece, file.piece)) || !sink.get ())) rc = -1;
  for (U64 off = 0 ; off < size && !rc ; off += file.piece)
    { const size_t n = size - off < file.piece ? (size_t) (size - off) : file.piece;
      rc = file.upload (fd, off, n, dPiece, 0, "mgBgzfDeflateFile");
      if (rc == -2) mgSetError ("failed to read file %s", inName);
      if (!rc && hipStreamSynchronize (0) != hipSuccess) { scratch.fail (); rc = -1; }
      if (!rc && mgBgzfSinkAppendDevice (sink.device (), dPiece, n)) rc = -1;
    }
  file.release ();
  ::close (fd);
  return sink.close (rc ? -1 : 0);
}
