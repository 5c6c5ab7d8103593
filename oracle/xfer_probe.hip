/* oracle/xfer_probe.hip — TEST INFRASTRUCTURE ONLY.
 *
 * libxferprobe.so: the three internal entry points of modimizer_amd/csrc/mg_xfer.h (mgXferD2H with its op, mgXferH2D, mgXferH2DSparse)
 * behind plain ones, so that tests/test_gpu_xfer.py can move arrays of its own choosing through the team of host threads: lengths
 * around the piece and around T pieces, pointers off their alignment, the saturating add across a piece edge, and host ranges the
 * sparse upload has to tell apart (never written, partly written, file-backed, shared).  The library's callers reach this code only
 * with the arrays a Modset or a Reference happens to have.
 *
 * Host code only, no kernel: the probe is LINKED against modimizer_amd/libmodgpu.so, so what runs is the library's own binary, not a
 * second compile of mg_xfer.hip.
 *
 * The transfers take the pointers as they are given (the device ones are the test's DeviceBuffers) and return the MgStatus.  The
 * mappings are made here so that the test knows what kind of memory it hands over: numpy's arrays are malloc ()ed, and what malloc ()
 * gives may have been written before.  The Makefile bakes a hash of this file, mg_xfer.h and mg_common.h into it (xfer_probe.inc);
 * xferProbeHash () returns it and the tests compare it with the tree's. */
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include "../modimizer_amd/csrc/mg_common.h"
#include "../modimizer_amd/csrc/mg_xfer.h"
#include "xfer_probe.inc"

static const char gProbeMarker[] = "XFER_PROBE_HASH=" XFER_PROBE_HASH;
extern "C" const char *xferProbeHash (void) { return gProbeMarker + 16; }

extern "C" int xferProbeD2H (void *hostDst, const void *devSrc, U64 bytes, int op) { return (int) mgXferD2H (hostDst, devSrc, (size_t) bytes, op); }
extern "C" int xferProbeH2D (void *devDst, const void *hostSrc, U64 bytes) { return (int) mgXferH2D (devDst, hostSrc, (size_t) bytes); }
extern "C" int xferProbeH2DSparse (void *devDst, const void *hostSrc, U64 bytes) { return (int) mgXferH2DSparse (devDst, hostSrc, (size_t) bytes); }

/* ---- host ranges (0: none to be had) ---- */

/* private anonymous memory that nobody has touched: what calloc () hands out for a large array */
extern "C" void *xferProbeMapAnon (U64 bytes)
{
  void *p = mmap (0, (size_t) bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  return p == MAP_FAILED ? 0 : p;
}

extern "C" void *xferProbeMapShared (U64 bytes)
{
  void *p = mmap (0, (size_t) bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  return p == MAP_FAILED ? 0 : p;
}

/* a temporary file of `bytes` bytes that depend on their place and on seed, written with write () and without a name by the time this
   returns: the descriptor (-1: none) */
static int xferProbeTempFile (U64 bytes, U64 seed)
{
  const char *dir = getenv ("TMPDIR");
  char path[4096];
  if (snprintf (path, sizeof path, "%s/xfer_probe_XXXXXX", dir && *dir ? dir : "/tmp") >= (int) sizeof path) return -1;
  const int fd = mkstemp (path);
  if (fd < 0) return -1;
  unlink (path);
  const size_t chunk = (size_t) 1 << 16;
  U8 *buf = (U8 *) malloc (chunk);
  bool ok = buf != 0;
  U64 x = seed * 0x9E3779B97F4A7C15ull + 1;
  for (U64 at = 0 ; ok && at < bytes ; )
    { const size_t len = bytes - at < chunk ? (size_t) (bytes - at) : chunk;
      for (size_t i = 0 ; i < len ; ++i) { x = x * 6364136223846793005ull + 1442695040888963407ull; buf[i] = (U8) ((x >> 56) | 1); }      /* (no zero byte: a page that arrives cleared shows) */
      for (size_t done = 0 ; ok && done < len ; )
        { const ssize_t w = write (fd, buf + done, len - done);
          if (w <= 0) ok = false; else done += (size_t) w;
        }
      at += len;
    }
  free (buf);
  if (!ok) { close (fd); return -1; }
  return fd;
}

/* a MAP_PRIVATE mapping of such a file: its pages have contents and none of them exists in this process until it is read */
extern "C" void *xferProbeMapFile (U64 bytes, U64 seed)
{
  const int fd = xferProbeTempFile (bytes, seed);
  if (fd < 0) return 0;
  void *p = mmap (0, (size_t) bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE, fd, 0);
  close (fd);
  return p == MAP_FAILED ? 0 : p;
}

/* an anonymous mapping of `bytes` whose second half (from the page at or behind bytes / 2 on) is replaced, MAP_FIXED, by a private
   mapping of such a file: one range, two kinds of memory */
extern "C" void *xferProbeMapHalfFile (U64 bytes, U64 seed)
{
  const size_t pg = (size_t) sysconf (_SC_PAGESIZE);
  const size_t half = ((size_t) bytes / 2 + pg - 1) / pg * pg;
  if (half >= bytes) return 0;
  char *p = (char *) xferProbeMapAnon (bytes);
  if (!p) return 0;
  const int fd = xferProbeTempFile (bytes - half, seed);
  if (fd < 0) { munmap (p, (size_t) bytes); return 0; }
  void *q = mmap (p + half, (size_t) bytes - half, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_FIXED, fd, 0);
  close (fd);
  if (q == MAP_FAILED) { munmap (p, (size_t) bytes); return 0; }
  return p;
}

/* asks the kernel to write the range's pages to swap (0: asked; where there is no swap they stay): a page that is swapped out is
   not present and still has contents, bit 62 of its pagemap entry says so */
extern "C" int xferProbePageOut (void *p, U64 bytes)
{
#ifdef MADV_PAGEOUT
  return madvise (p, (size_t) bytes, MADV_PAGEOUT);
#else
  (void) p; (void) bytes; return -1;
#endif
}

extern "C" int xferProbeUnmap (void *p, U64 bytes) { return munmap (p, (size_t) bytes); }

/* which pages of [addr, addr + bytes) exist, by /proc/self/pagemap (bit 63: present, bit 62: swapped): out[i] = 1 or 0 for the i-th
   page the range touches (a byte a page, (addr + bytes - 1) / page - addr / page + 1 of them); the number that exist, -1 if the file
   cannot be read */
extern "C" long xferProbePresentPages (const void *addr, U64 bytes, U8 *out)
{
  if (!bytes) return 0;
  const size_t pg = (size_t) sysconf (_SC_PAGESIZE);
  const size_t a0 = (size_t) addr, first = a0 / pg, n = (a0 + (size_t) bytes - 1) / pg - first + 1;
  const int fd = open ("/proc/self/pagemap", O_RDONLY);
  if (fd < 0) return -1;
  U64 ent[512];
  long present = 0;
  for (size_t p = 0 ; p < n ; )
    { const size_t want = n - p < 512 ? n - p : 512;
      for (size_t got = 0 ; got < want * 8 ; )
        { const ssize_t r = pread (fd, (char *) ent + got, want * 8 - got, (off_t) ((first + p) * 8 + got));
          if (r <= 0) { close (fd); return -1; }
          got += (size_t) r;
        }
      for (size_t i = 0 ; i < want ; ++i) { const U8 e = (U8) ((ent[i] >> 62) != 0); if (out) out[p + i] = e; present += e; }
      p += want;
    }
  close (fd);
  return present;
}
