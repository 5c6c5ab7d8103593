#!/bin/bash
# dev: the reports' writer (mg_textout.c MgTextOut: page-locked blocks filled on the caller's thread, a writer thread behind it) under
# ThreadSanitizer, then under AddressSanitizer + UBSan, on the CPU with host memory as the "device": three calls of 40 MiB of a counter
# pattern -- each crosses MG_TOUT_PIECE (32 MiB), and their six pieces outnumber the four blocks, so the caller waits for the writer --
# then a call of 5 bytes, which reuses a large block for a small piece; the file is compared with the pattern.
# Compiled: mg_textout.c + mg_knobs.c.  Writes under $TMPDIR.
set -e
R=$(cd "$(dirname "$0")/.." && pwd); D=${TMPDIR:-/tmp}/modgpu_tsan_textout; mkdir -p $D
cat > $D/main.c <<'EOS'
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "modgpu.h"
#include "mg_internal.h"
/* "device" memory is host memory here */
MgStatus mgMemcpyD2H (void *d, const void *s, size_t n, void *st) { (void) st; memcpy (d, s, n); return MG_OK; }
void *mgPinnedAlloc (size_t n) { return malloc (n ? n : 16); } void mgPinnedFree (void *p) { free (p); }
const char *mgLastError (void) { return "stub"; }
/* byte x of the stream: the top byte of a 64-bit mix of x, which depends on every bit of x -- no period, so a piece that lands at the wrong place,
   or is filled from the wrong offset, differs from what belongs there */
static void pattern (unsigned char *p, size_t n, unsigned long long from)
{ for (size_t i = 0 ; i < n ; ++i) p[i] = (unsigned char) ((from + i) * 0x9E3779B97F4A7C15ull >> 56); }
int main (int argc, char **argv)
{ const char *path = argv[1]; (void) argc;
  const size_t big = (size_t) 40 << 20;
  unsigned char *src = malloc (big), *back = malloc (big);
  FILE *out = fopen (path, "wb");
  if (!src || !back || !out) return 2;
  MgTextOut *w = mgTextOutOpen (out);
  unsigned long long at = 0;
  for (int c = 0 ; c < 4 ; ++c)
    { const size_t n = c < 3 ? big : 5;
      pattern (src, n, at);
      if (mgTextOutFromDevice (w, src, n)) { fprintf (stderr, "copy failed\n"); return 1; }      /* (src is the caller's again when it returns) */
      at += n;
    }
  if (mgTextOutClose (w)) { fprintf (stderr, "write failed\n"); return 1; }
  if (fclose (out)) return 1;
  FILE *in = fopen (path, "rb"); unsigned long long seen = 0;
  for (;;)
    { const size_t n = fread (back, 1, big, in);
      if (!n) break;
      pattern (src, n, seen);
      if (memcmp (src, back, n)) { fprintf (stderr, "file differs from the pattern after byte %llu\n", seen); return 1; }
      seen += n;
    }
  fclose (in);
  if (seen != at) { fprintf (stderr, "file holds %llu bytes, %llu written\n", seen, at); return 1; }
  printf ("textout ok: %llu bytes\n", at);
  free (src); free (back); return 0; }
EOS
for san in thread address,undefined; do
  gcc -g -O1 -fsanitize=$san -fno-sanitize-recover=all -std=gnu11 -I$R/include -I$R/modimizer_amd/csrc -o $D/t $D/main.c \
      $R/modimizer_amd/csrc/mg_textout.c $R/modimizer_amd/csrc/mg_knobs.c -lpthread
  $D/t $D/out.bin
  echo "  -fsanitize=$san: output identical ($(wc -c < $D/out.bin) bytes)"
done
rm -f $D/out.bin
