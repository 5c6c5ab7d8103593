/* deflate_host_check.c -- the encoder of csrc/mg_deflate_core.h by itself, for guard pages and the sanitizers:
 *
 *   cc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I modimizer_amd/csrc tools/deflate_host_check.c -o deflate_host_check
 *   ./deflate_host_check corpus.bin          (tests/test_deflate_host.py write_corpus () makes the file; tools/asan_deflate.sh does all three;
 *                                             the test of that module runs the program built without the sanitizers)
 *
 * Plain host code with its own main: it includes nothing of the library but the two core headers (the encoder takes the CRC-32 from the
 * decoder's).  Every text of the corpus -- a count, then per text its length as a little-endian word and its bytes -- is deflated twice
 * between inaccessible guard pages: once with the text ending at the page after it, once with it starting at the page before it, read-only
 * both times; the 65536-byte slot is whole pages, so a guard page lies directly before and directly after it in both runs, and the token
 * list of exactly n words ends at (begins behind) a guard page too.  A single byte read or written outside any range faults.  Prints
 * "block I len L crc C kind K" per text, C being the CRC-32 of the member's bytes; exit status 1 if the two runs disagree. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include "mg_deflate_core.h"

typedef struct { uint8_t *map, *p; size_t span, body; } Guarded;

static Guarded guarded (size_t n, int atEnd)
{
  const size_t page = (size_t) sysconf (_SC_PAGESIZE);
  Guarded g;
  g.body = (n + page - 1) / page * page; if (!g.body) g.body = page;
  g.span = g.body + 2 * page;
  g.map = (uint8_t *) mmap (0, g.span, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (g.map == MAP_FAILED) { perror ("mmap"); exit (2); }
  memset (g.map + page, 0xA5, g.body);
  if (mprotect (g.map, page, PROT_NONE) || mprotect (g.map + page + g.body, page, PROT_NONE)) { perror ("mprotect"); exit (2); }
  g.p = atEnd ? g.map + page + g.body - n : g.map + page;
  return g;
}

static uint32_t crcOf (const uint8_t *p, uint32_t n)
{
  static uint32_t tab[256];
  uint32_t c = 0, lane;
  mgInfCrcTable (tab, 0, 1);
  for (lane = 0 ; lane < MGI_LANES ; ++lane) c ^= mgInfCrcSlice (tab, p, n, lane);
  return c;
}

int main (int argc, char **argv)
{
  if (argc != 2) { fprintf (stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE *f = fopen (argv[1], "rb");
  if (!f) { perror (argv[1]); return 2; }
  uint32_t n = 0, bad = 0;
  if (fread (&n, 4, 1, f) != 1) { fprintf (stderr, "short corpus\n"); return 2; }
  const size_t page = (size_t) sysconf (_SC_PAGESIZE);
  MgDefWork *W = (MgDefWork *) malloc (sizeof (MgDefWork));
  if (!W) return 2;
  for (uint32_t i = 0 ; i < n ; ++i)
    { uint32_t uLen = 0;
      if (fread (&uLen, 4, 1, f) != 1 || uLen > MGD_BLOCK_MAX) { fprintf (stderr, "short corpus\n"); return 2; }
      uint8_t *text = (uint8_t *) malloc (uLen ? uLen : 1);
      if (!text || fread (text, 1, uLen, f) != uLen) { fprintf (stderr, "short corpus\n"); return 2; }
      uint32_t len[2], crc[2];
      uint64_t kind[2];
      for (int side = 0 ; side < 2 ; ++side)
        { Guarded t = guarded (uLen, side), o = guarded (MGD_SLOT, side), k = guarded ((size_t) uLen * 4, side);
          uint64_t stats[8] = { 0 };
          memcpy (t.p, text, uLen);
          if (mprotect (t.map + page, t.body, PROT_READ)) { perror ("mprotect"); return 2; }      /* the encoder only reads its text */
          len[side] = mgDefMember (t.p, uLen, o.p, (uint32_t *) (void *) k.p, W, 0, 1, stats);
          if (len[side] > MGD_SLOT) { printf ("block %u: a member of %u bytes\n", i, len[side]); ++bad; len[side] = MGD_SLOT; }
          crc[side] = crcOf (o.p, len[side]); kind[side] = stats[MGD_ST_KIND];
          munmap (t.map, t.span); munmap (o.map, o.span); munmap (k.map, k.span);
        }
      if (len[0] != len[1] || crc[0] != crc[1] || kind[0] != kind[1]) { printf ("block %u: the two runs disagree (%u, %u)\n", i, len[0], len[1]); ++bad; }
      printf ("block %u len %u crc %08x kind %u\n", i, len[0], crc[0], (unsigned) kind[0]);
      free (text);
    }
  free (W);
  fclose (f);
  printf ("%u blocks, %u bad\n", n, bad);
  return bad ? 1 : 0;
}
