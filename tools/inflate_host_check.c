/* inflate_host_check.c -- the decoder of csrc/mg_inflate_core.h by itself, for the sanitizers:
 *
 *   cc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I modimizer_amd/csrc tools/inflate_host_check.c -o inflate_host_check
 *   ./inflate_host_check corpus.bin          (tests/test_inflate_host.py write_corpus () makes the file; tools/asan_inflate.sh does all three;
 *                                             the test of that module runs the program built without the sanitizers)
 *
 * Plain host code with its own main: it includes nothing of the library but that header.  Every member of the corpus -- a count, then per
 * member cLen, uLen, crc as little-endian words and the payload -- is inflated twice between inaccessible guard pages: once with the payload
 * and the output range ending at the page after them, once with both starting at the page before them, so a single byte read or written
 * outside either range faults.  The rest of the output's pages is 0xA5 and must still be.  Prints "member I status S crc C" per member;
 * exit status 1 if the two runs disagree or a guard byte changed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include "mg_inflate_core.h"

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

int main (int argc, char **argv)
{
  if (argc != 2) { fprintf (stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE *f = fopen (argv[1], "rb");
  if (!f) { perror (argv[1]); return 2; }
  uint32_t n = 0, bad = 0;
  if (fread (&n, 4, 1, f) != 1) { fprintf (stderr, "short corpus\n"); return 2; }
  const size_t page = (size_t) sysconf (_SC_PAGESIZE);
  for (uint32_t i = 0 ; i < n ; ++i)
    { uint32_t head[3];
      if (fread (head, 4, 3, f) != 3) { fprintf (stderr, "short corpus\n"); return 2; }
      const uint32_t cLen = head[0], uLen = head[1], crc = head[2];
      uint8_t *pay = (uint8_t *) malloc (cLen ? cLen : 1);
      if (!pay || fread (pay, 1, cLen, f) != cLen) { fprintf (stderr, "short corpus\n"); return 2; }
      uint32_t status[2], sum[2];
      for (int side = 0 ; side < 2 ; ++side)
        { Guarded c = guarded (cLen, side), o = guarded (uLen, side);
          MgInfTables T;
          uint64_t stats[8] = { 0 };
          memcpy (c.p, pay, cLen);
          if (mprotect (c.map + page, c.body, PROT_READ)) { perror ("mprotect"); return 2; }      /* the decoder only reads its input */
          status[side] = mgInfMember (c.p, cLen, o.p, uLen, crc, &T, stats);
          sum[side] = 0;
          for (uint32_t k = 0 ; k < uLen ; ++k) sum[side] = sum[side] * 31 + o.p[k];
          for (uint8_t *q = o.map + page ; q < o.map + page + o.body ; ++q)
            if ((q < o.p || q >= o.p + uLen) && *q != 0xA5) { printf ("member %u: a byte outside the output range was written\n", i); ++bad; break; }
          munmap (c.map, c.span); munmap (o.map, o.span);
        }
      if (status[0] != status[1] || (!status[0] && sum[0] != sum[1])) { printf ("member %u: the two runs disagree (%u, %u)\n", i, status[0], status[1]); ++bad; }
      printf ("member %u status %u crc %08x\n", i, status[0], crc);
      free (pay);
    }
  fclose (f);
  printf ("%u members, %u bad\n", n, bad);
  return bad ? 1 : 0;
}
