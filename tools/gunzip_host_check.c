/* gunzip_host_check.c -- the gzip pipeline of csrc/mg_gunzip_core.h by itself, for the sanitizers:
 *
 *   cc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I modimizer_amd/csrc tools/gunzip_host_check.c -o gunzip_host_check
 *   ./gunzip_host_check corpus.bin          (tests/test_gunzip_host.py write_corpus () makes the file; the test of that module runs the program
 *                                             built without the sanitizers)
 *
 * Plain host code with its own main: it includes nothing of the library but that header (and through it mg_inflate_core.h).  Every run of the
 * corpus -- a count, then per run chunk bytes, batch chunks, symbols per chunk, the output's capacity and the file's length as little-endian
 * words, and the gzip file -- goes through mgzNext / mgzBatchHost twice between inaccessible guard pages: once with the file and the output range
 * ending at the page after them, once with both starting at the page before them, so a single byte read or written outside either range faults.
 * The batch's own arrays (chunk records, symbols, windows) come from malloc at their exact sizes, which is what AddressSanitizer watches.
 * Prints "run I status S len L crc C diag D0 .. D7" per run; exit status 1 if the two runs disagree or a guard byte changed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include "mg_gunzip_core.h"

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

typedef struct { MgzHostMem M; uint8_t *out; uint64_t produced; MgInfTables T; } Run;

static uint32_t peek (void *v, uint64_t off, uint8_t *buf, uint32_t n)
{
  const Run *r = (const Run *) v;
  if (off >= r->M.n) return 0;
  if (r->M.n - off < n) n = (uint32_t) (r->M.n - off);
  memcpy (buf, r->M.comp + off, n);
  return n;
}
/* the arrays at exactly the sizes the plan asks for, fresh for every batch but for the window the stream carries in slot 0 */
static int batch (void *v, const MgzPlan *P, MgzSummary *S)
{
  Run *r = (Run *) v;
  uint8_t carry[MGZ_WINDOW];
  if (r->M.win) memcpy (carry, r->M.win, MGZ_WINDOW); else memset (carry, 0, MGZ_WINDOW);
  free (r->M.ch); free (r->M.sym); free (r->M.win);
  r->M.ch = (MgzChunk *) malloc ((size_t) P->nChunks * sizeof (MgzChunk));
  r->M.sym = (uint16_t *) malloc ((size_t) P->nChunks * P->cap * sizeof (uint16_t));
  r->M.win = (uint8_t *) malloc (((size_t) P->nChunks + 1) * MGZ_WINDOW);
  if (!r->M.ch || !r->M.sym || !r->M.win) { fprintf (stderr, "no memory\n"); exit (2); }
  memcpy (r->M.win, carry, MGZ_WINDOW);
  r->M.out = r->out + r->produced; r->M.T = &r->T;
  mgzBatchHost (&r->M, P, S);
  r->produced += S->outBytes;
  return 0;
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
    { uint32_t head[5];
      if (fread (head, 4, 5, f) != 5) { fprintf (stderr, "short corpus\n"); return 2; }
      const uint32_t chunk = head[0], nBatch = head[1], spc = head[2], cap = head[3], cLen = head[4];
      uint8_t *file = (uint8_t *) malloc (cLen ? cLen : 1);
      if (!file || fread (file, 1, cLen, f) != cLen) { fprintf (stderr, "short corpus\n"); return 2; }
      uint32_t status[2], sum[2], crc[2];
      uint64_t len[2], diag[2][8];
      for (int side = 0 ; side < 2 ; ++side)
        { Guarded c = guarded (cLen, side), o = guarded (cap, side);
          Run r; memset (&r, 0, sizeof (r));
          MgzStream st;
          int rc = 0;
          memcpy (c.p, file, cLen);
          if (mprotect (c.map + page, c.body, PROT_READ)) { perror ("mprotect"); return 2; }      /* the pipeline only reads its input */
          r.M.comp = c.p; r.M.n = cLen; r.out = o.p;
          mgzStreamInit (&st, cLen, chunk, nBatch, spc, cap);
          while (!st.done && !rc) rc = mgzNext (&st, peek, batch, &r);
          status[side] = st.status; len[side] = st.produced; memcpy (diag[side], st.diag, sizeof (st.diag));
          sum[side] = 0; crc[side] = 0xffffffffu;
          mgInfCrcTable (r.T.crcTab, 0, 1);
          for (uint64_t k = 0 ; k < st.produced ; ++k) { sum[side] = sum[side] * 31 + o.p[k]; crc[side] = r.T.crcTab[(crc[side] ^ o.p[k]) & 0xff] ^ (crc[side] >> 8); }
          if (st.produced > cap) { printf ("run %u: more text than the output holds\n", i); ++bad; }
          for (uint8_t *q = o.map + page ; q < o.map + page + o.body ; ++q)
            if ((q < o.p || q >= o.p + cap) && *q != 0xA5) { printf ("run %u: a byte outside the output range was written\n", i); ++bad; break; }
          free (r.M.ch); free (r.M.sym); free (r.M.win);
          munmap (c.map, c.span); munmap (o.map, o.span);
        }
      if (status[0] != status[1] || len[0] != len[1] || sum[0] != sum[1] || memcmp (diag[0], diag[1], sizeof (diag[0])))
        { printf ("run %u: the two runs disagree (%u, %u)\n", i, status[0], status[1]); ++bad; }
      printf ("run %u status %u len %llu crc %08x diag", i, status[0], (unsigned long long) len[0], crc[0] ^ 0xffffffffu);
      for (int k = 0 ; k < 8 ; ++k) printf (" %llu", (unsigned long long) diag[0][k]);
      printf ("\n");
      free (file);
    }
  fclose (f);
  printf ("%u runs, %u bad\n", n, bad);
  return bad ? 1 : 0;
}
