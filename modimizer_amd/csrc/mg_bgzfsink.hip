/* mg_bgzfsink.hip — text ON THE DEVICE written as a blocked-gzip (BGZF) file: the mirror of mg_bgzfsrc.hip.  Producers append to a device row
 * of text -- a device range (device-to-device copy), a run of one byte value (hipMemsetAsync; FASTA -> FASTQ splices runs of '!' that can be
 * longer than a window), a few host bytes -- and whenever the row is full its whole blocks of MODGPU_BGZF_BLOCK bytes (default and at most
 * 65280, bgzip's) are deflated by the kernel of mg_deflate.hip, one member a block, packed, and handed to `emit` as ONE device range: the
 * caller copies it to a page-locked block and gives it to its writer thread.  What crosses the link is the file's bytes and nothing else.
 * The tail of less than one block stays on the device, at the front of the row; close deflates it as a short member and emits bgzip's 28-byte
 * end-of-file member.
 *
 * The file's bytes do not depend on how the producers cut their appends, nor on the row's size: member k is the encoding of bytes
 * [k * block, (k + 1) * block) of the whole text, and a member is a pure function of its block (mg_deflate_core.h).
 *
 * Everything runs on a stream of the sink's own and every call returns with its work over: an appended range may be reused at once, and
 * `emit` has the packed members to itself until it returns. */
#include <string.h>
#include <vector>
#include "mg_common.h"
#include "mg_internal.h"
#include "mg_deflate_core.h"

#define SK_ROW_BLOCKS 1024u                              /* blocks of a full row: a launch with several blocks for every CU */
#define SK_MEMBER_EXTRA 31u                              /* a member is at most its block's bytes + header, stored-block header and trailer: the encoder never writes more than the stored form */

struct MgBgzfSink {
  MgBgzfEmitFn emit = 0; void *ctx = 0; const char *what = "";
  U32 block = MGD_BLOCK_MAX, rowBlocks = 1;
  size_t rowCap = 0, packedCap = 0, have = 0;
  unsigned char *dRow = 0, *dPacked = 0; hipStream_t st = 0;
  MgDeflateWork *work = 0;
  std::vector<MgGzBlock> tab; std::vector<U64> off;
  bool failed = false;
};

static int skHip (MgBgzfSink *s) { s->failed = true; mgHipFail (hipGetLastError (), s->what); return -1; }

extern "C" size_t mgBgzfSinkEmitMax (const MgBgzfSink *s) { return s->packedCap; }

extern "C" MgBgzfSink *mgBgzfSinkOpen (MgBgzfEmitFn emit, void *ctx, const char *what, U64 textHint)
{
  MgBgzfSink *s = new MgBgzfSink;
  s->emit = emit; s->ctx = ctx; s->what = what ? what : "blocked gzip on the device";
  const long k = mgKnobs ()->bgzfBlock;
  s->block = k >= 1 && k <= (long) MGD_BLOCK_MAX ? (U32) k : MGD_BLOCK_MAX;
  const U64 blocks = textHint ? (textHint + s->block - 1) / s->block : SK_ROW_BLOCKS;
  s->rowBlocks = blocks < SK_ROW_BLOCKS ? (U32) blocks : SK_ROW_BLOCKS;
  s->rowCap = (size_t) s->rowBlocks * s->block;
  s->packedCap = (size_t) s->rowBlocks * (s->block + SK_MEMBER_EXTRA) + MGD_EOF_BYTES;
  s->work = mgDeflateWorkNew ();
  if (hipStreamCreateWithFlags (&s->st, hipStreamNonBlocking) != hipSuccess || hipMalloc ((void **) &s->dRow, s->rowCap) != hipSuccess
      || hipMalloc ((void **) &s->dPacked, s->packedCap) != hipSuccess)
    { mgHipFail (hipGetLastError (), s->what); (void) mgBgzfSinkClose (s, 0); return 0; }
  return s;
}

/* the row's whole blocks -- and, at the end, its tail -- deflated and emitted; the tail of less than a block to the row's front */
static int skFlush (MgBgzfSink *s, bool final)
{
  const U32 whole = (U32) (s->have / s->block), rest = (U32) (s->have % s->block), n = whole + (final && rest ? 1u : 0u);
  if (!n) return 0;
  s->tab.resize (n); s->off.resize ((size_t) n + 1);
  for (U32 i = 0 ; i < n ; ++i) { s->tab[i].uOff = (U64) i * s->block; s->tab[i].uLen = i < whole ? s->block : rest; s->tab[i].pad = 0; }
  if (mgDeflateRun (s->work, s->dRow, s->have, s->tab.data (), n, s->dPacked, s->packedCap, s->off.data (), (void *) s->st) != MG_OK) { s->failed = true; return -1; }
  if (s->emit (s->ctx, s->dPacked, (size_t) s->off[n], 1, (void *) s->st)) { s->failed = true; return -1; }
  if (n > whole) s->have = 0;
  else
    { if (rest && (hipMemcpyAsync (s->dRow, s->dRow + (size_t) whole * s->block, rest, hipMemcpyDeviceToDevice, s->st) != hipSuccess      /* (whole >= 1: the two ranges lie apart) */
                   || hipStreamSynchronize (s->st) != hipSuccess)) return skHip (s);
      s->have = rest;
    }
  return 0;
}

/* kind 0: a device range, 1: host bytes, 2: a run of byte `value` */
static int skAppend (MgBgzfSink *s, int kind, const unsigned char *src, int value, U64 n)
{
  if (s->failed) return mgFailedWith ("blocked gzip on the device: an earlier append failed");
  while (n)
    { const size_t room = s->rowCap - s->have, take = n < room ? (size_t) n : room;
      const hipError_t e = kind == 2 ? hipMemsetAsync (s->dRow + s->have, value, take, s->st)
                                     : hipMemcpyAsync (s->dRow + s->have, src, take, kind ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s->st);
      if (e != hipSuccess || hipStreamSynchronize (s->st) != hipSuccess) return skHip (s);
      s->have += take; n -= take; if (src) src += take;
      if (s->have == s->rowCap && skFlush (s, false)) return -1;
    }
  return 0;
}
extern "C" int mgBgzfSinkAppendDevice (MgBgzfSink *s, const unsigned char *dSrc, size_t n) { return skAppend (s, 0, dSrc, 0, n); }
extern "C" int mgBgzfSinkAppendHost (MgBgzfSink *s, const void *p, size_t n) { return skAppend (s, 1, (const unsigned char *) p, 0, n); }
extern "C" int mgBgzfSinkAppendRun (MgBgzfSink *s, int byte, U64 n) { return skAppend (s, 2, 0, byte, n); }

extern "C" int mgBgzfSinkClose (MgBgzfSink *s, int flush)
{
  int rc = 0;
  if (!s) return 0;
  if (flush)
    { unsigned char eof[MGD_EOF_BYTES];
      mgDefEofMember (eof);
      if (s->failed || skFlush (s, true) || s->emit (s->ctx, eof, sizeof (eof), 0, (void *) s->st)) rc = mgFailedWith ("blocked gzip on the device: the file is not complete");
    }
  if (s->st) { (void) hipStreamSynchronize (s->st); (void) hipStreamDestroy (s->st); }
  (void) hipFree (s->dRow); (void) hipFree (s->dPacked);
  mgDeflateWorkFree (s->work);
  delete s;
  return rc;
}
