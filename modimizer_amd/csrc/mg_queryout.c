/* mg_queryout.c — modmap's "Q" / "M" lines on their way out: the hand-written formatter and its team, the block pool behind its
 * buffers, and the three-stage pipe of the file entry point (device half, formatter, writer).
 *
 * A short-read query file is tens of millions of lines a second at the rate the kernels deliver the tallies, and fprintf does
 * three to five million: the lines of a batch are formatted into per-thread buffers by hand-written conversions and written out
 * in order.  "%d", "%llu", "%s" are what they are; "%.2f" is glibc's: the double's EXACT binary value rounded to two decimals,
 * ties to even -- done here in integer arithmetic on the mantissa (x = m * 2^e, so 100 x = 100 m * 2^e exactly; the quotient
 * and remainder of the shift decide), with snprintf itself for what never occurs at speed (nan from 0 / 0, inf, negative).
 */
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <pthread.h>
#include "modgpu.h"
#include "mg_internal.h"

static char *fmtU (char *p, unsigned long long v)
{ char t[24]; int n = 0; do { t[n++] = (char) ('0' + v % 10); v /= 10; } while (v); while (n) *p++ = t[--n]; return p; }
static char *fmtI (char *p, long long v) { if (v < 0) { *p++ = '-'; return fmtU (p, (unsigned long long) (-(v + 1)) + 1); } return fmtU (p, (unsigned long long) v); }
static char *fmtS (char *p, const char *s) { size_t n = strlen (s); memcpy (p, s, n); return p + n; }
static char *fmtF2 (char *p, double x)
{
  if (!(x >= 0) || x >= 1e15 || signbit (x)) return p + snprintf (p, 48, "%.2f", x);
  int e; const double fr = frexp (x, &e);                              /* x = fr * 2^e, 0.5 <= fr < 1 (or x == 0) */
  const unsigned long long mant = (unsigned long long) ldexp (fr, 53);   /* exact: 53 bits */
  const int s = 53 - e;                                                /* x = mant * 2^-s; x < 1e15 < 2^50, so s >= 3 */
  const unsigned long long v = mant * 100;                             /* < 2^60 */
  unsigned long long q = 0;
  if (s < 64)
    { q = v >> s;
      const unsigned long long rem = v & ((1ull << s) - 1), half = 1ull << (s - 1);
      if (rem > half || (rem == half && (q & 1))) ++q;
    }
  const unsigned long long whole = (unsigned long long) (q / 100); const unsigned frac = (unsigned) (q % 100);
  p = fmtU (p, whole); *p++ = '.'; *p++ = (char) ('0' + frac / 10); *p++ = (char) ('0' + frac % 10);
  return p;
}

int mgFormatF2 (char *buf, double x) { char *e = fmtF2 (buf, x); *e = 0; return (int) (e - buf); }      /* test hook: buf of 64 bytes */

/* the buffers of the output stages -- the teams' pieces, the ids that travel with a batch -- come from a small pool and go back to
   it: a fresh 2 MB block from malloc () is 500 page faults when it is written, by sixteen threads at once, and as many pages given
   back when it is freed; 4e6 lines a batch-sequence are 57 000 of each.  The pool keeps up to MG_POOL_SLOTS blocks between calls
   (mgReleaseBuffers () frees them); a block remembers its capacity in the 16 bytes in front of it. */
#define MG_POOL_SLOTS 128
static struct { pthread_mutex_t mu; void *blk[MG_POOL_SLOTS]; int n; } gPool = { PTHREAD_MUTEX_INITIALIZER, { 0 }, 0 };
static size_t poolCap (const void *p) { return *(const size_t *) ((const char *) p - 16); }
static void *poolGet (size_t bytes)
{
  void *hit = 0;
  pthread_mutex_lock (&gPool.mu);
  int pick = -1;
  for (int i = 0 ; i < gPool.n ; ++i)
    { const size_t c = poolCap (gPool.blk[i]);
      if (c >= bytes && (pick < 0 || c < poolCap (gPool.blk[pick]))) pick = i;      /* the tightest fit */
    }
  if (pick >= 0) { hit = gPool.blk[pick]; gPool.blk[pick] = gPool.blk[--gPool.n]; }
  pthread_mutex_unlock (&gPool.mu);
  if (hit) return hit;
  const size_t cap = bytes + bytes / 8 + 64;
  char *raw = (char *) malloc (cap + 16);
  if (!raw) mgFatal ("out of memory");
  *(size_t *) raw = cap;
  return raw + 16;
}
static void poolPut (void *p)
{
  if (!p) return;
  pthread_mutex_lock (&gPool.mu);
  if (gPool.n < MG_POOL_SLOTS) { gPool.blk[gPool.n++] = p; p = 0; }
  pthread_mutex_unlock (&gPool.mu);
  if (p) free ((char *) p - 16);
}
static void *poolGrow (void *p, size_t keep, size_t bytes)  /* a block of at least `bytes` holding the first `keep` bytes of p */
{
  void *q = poolGet (bytes);
  if (keep) memcpy (q, p, keep);
  poolPut (p);
  return q;
}
static void poolFreeAll (void)
{
  pthread_mutex_lock (&gPool.mu);
  for (int i = 0 ; i < gPool.n ; ++i) free ((char *) gPool.blk[i] - 16);
  gPool.n = 0;
  pthread_mutex_unlock (&gPool.mu);
}

typedef struct { char *buf; size_t len, cap; } FmtBuf;      /* buf: a pool block */
static char *fmtRoom (FmtBuf *b, size_t need)
{ if (b->len + need > b->cap) { b->buf = (char *) poolGrow (b->buf, b->len, 2 * (b->len + need) + 4096); b->cap = poolCap (b->buf); } return b->buf + b->len; }
typedef struct { const MgReference *ref; const MgChainQ *q; const MgChainM *m; const U64 *mStart; const int64_t *offsets; const char **names; int r0, r1; FmtBuf out; double cpuMs; } FmtJob;
static void *fmtQM (void *v)
{
  FmtJob *j = (FmtJob *) v;
  struct timespec u0, u1; clock_gettime (CLOCK_THREAD_CPUTIME_ID, &u0);
  j->out.buf = (char *) poolGet ((size_t) (j->r1 - j->r0) * 80 + 4096); j->out.cap = poolCap (j->out.buf);      /* a Q line of a short read is 60 bytes */
  for (int r = j->r0 ; r < j->r1 ; ++r)
    { const MgChainQ *qq = &j->q[r];
      const char *nm = j->names[r]; const size_t nl = strlen (nm);
      char *p0 = fmtRoom (&j->out, 256 + nl), *p = p0;
      *p++ = 'Q'; *p++ = '\t'; memcpy (p, nm, nl); p += nl; *p++ = '\t';
      p = fmtU (p, (unsigned long long) (j->offsets[r + 1] - j->offsets[r])); *p++ = '\t';
      p = fmtI (p, (int) qq->missed); p = fmtS (p, " miss, "); p = fmtI (p, (int) qq->copy1); p = fmtS (p, " copy1, ");
      p = fmtI (p, (int) qq->copy2); p = fmtS (p, " copy2, "); p = fmtI (p, (int) qq->copyM); p = fmtS (p, " multi, ");
      p = fmtF2 (p, ((int) qq->nSeeds - (int) qq->missed) / (double) ((int) qq->nSeeds)); p = fmtS (p, " hit\n");
      j->out.len += (size_t) (p - p0);
      for (U32 k = 0 ; k < qq->nM ; ++k)
        { const MgChainM *e = &j->m[j->mStart[r] + k];
          const char *rn = j->ref->names[e->id0];
          p0 = fmtRoom (&j->out, 320 + nl + strlen (rn)); p = p0;
          *p++ = 'M'; *p++ = '\t'; memcpy (p, nm, nl); p += nl; *p++ = '\t';
          p = fmtI (p, (int) e->pos0); *p++ = '\t'; p = fmtI (p, (int) e->posN); *p++ = '\t'; p = fmtI (p, (int) (e->posN - e->pos0)); *p++ = '\t';
          p = fmtS (p, rn); *p++ = '\t'; p = fmtI (p, (int) e->off0); *p++ = '\t'; p = fmtI (p, (int) e->offN); *p++ = '\t';
          p = fmtI (p, e->n1); *p++ = ' '; p = fmtI (p, e->n2); *p++ = '\t';
          p = fmtF2 (p, (e->n1 + e->n2) / (double) e->span); *p++ = '\t';
          p = fmtF2 (p, e->n1 / (double) (int) qq->copy1); *p++ = '\n';
          j->out.len += (size_t) (p - p0);
        }
    }
  clock_gettime (CLOCK_THREAD_CPUTIME_ID, &u1);
  j->cpuMs = mgMsBetween (&u0, &u1);
  return 0;
}

static int fmtThreads (int nReads)
{
  if (nReads < 20000) return 1;
  long v = mgCpuBudget ();
  const long pk = mgKnobs ()->parseThreads; if (pk != MG_KNOB_UNSET && pk > 0) v = pk;
  if (v > 16) v = 16;
  if (v < 1) v = 1;
  return (int) v;
}

/* the lines of a batch whose tallies and blocks are on the host: formatted by a team of threads, each its range of the reads
   into its own buffer (piece[0 .. *nPieces)), and written in order.  (Positioned writes of the pieces by the team itself were tried:
   writes to one file take turns on its inode lock, 234 MB take the 40 ms one fwrite takes.) */
static void queryFormatLines (const MgReference *ref, const MgChainQ *q, const MgChainM *m, const int64_t *offsets, int nReads, const char **names,
                              FmtBuf piece[16], int *nPieces, double *ms, double *cpuMs)
{
  struct timespec c1, c2; clock_gettime (CLOCK_MONOTONIC, &c1);
  U64 *mStart = (U64 *) poolGet (((size_t) nReads + 1) * 8);
  { U64 tot = 0; for (int r = 0 ; r < nReads ; ++r) { mStart[r] = tot; tot += q[r].nM; } mStart[nReads] = tot; }
  const int T = fmtThreads (nReads);
  FmtJob job[16];
  for (int t = 0 ; t < T ; ++t)
    { memset (&job[t], 0, sizeof (FmtJob));
      job[t].ref = ref; job[t].q = q; job[t].m = m; job[t].mStart = mStart; job[t].offsets = offsets; job[t].names = names;
      job[t].r0 = (int) ((int64_t) nReads * t / T); job[t].r1 = (int) ((int64_t) nReads * (t + 1) / T);
    }
  mgTeamRun (T, fmtQM, job, sizeof (FmtJob));
  for (int t = 0 ; t < T ; ++t) { piece[t] = job[t].out; if (cpuMs) *cpuMs += job[t].cpuMs; }
  *nPieces = T;
  poolPut (mStart);
  clock_gettime (CLOCK_MONOTONIC, &c2);
  if (ms) *ms += mgMsBetween (&c1, &c2);
}
static void queryWritePieces (FmtBuf piece[16], int nPieces, FILE *out, double *ms)
{
  struct timespec c1, c2; clock_gettime (CLOCK_MONOTONIC, &c1);
  for (int t = 0 ; t < nPieces ; ++t)
    { if (piece[t].len && fwrite (piece[t].buf, 1, piece[t].len, out) != piece[t].len) mgFatal ("write");
      poolPut (piece[t].buf); piece[t].buf = 0;
    }
  clock_gettime (CLOCK_MONOTONIC, &c2);
  if (ms) *ms += mgMsBetween (&c1, &c2);
}

int mgQueryLinesOut (const MgReference *ref, const MgChainQ *q, const MgChainM *m, const int64_t *offsets, int nReads, const char **names, FILE *out,
                     double *msFormat, double *msWrite)
{
  FmtBuf piece[16]; int nPieces = 0;
  queryFormatLines (ref, q, m, offsets, nReads, names, piece, &nPieces, msFormat, 0);
  queryWritePieces (piece, nPieces, out, msWrite);
  return nPieces;
}

/* ---- the file entry point's batches: three stages, three threads ----
 * mgQueryFile hands over a batch per window of the file.  Push runs the device half (scan, lookups, tallies, chaining, the copies
 * to the host) on the caller's thread -- which goes on to read, parse and query the next window -- and queues the rest: a
 * FORMATTER thread (with its team) turns a batch's tallies and blocks into lines, a WRITER thread puts them out; batches pass
 * through both in order, at most two waiting in front of each.  A batch that needs the long way (-v, a read with more blocks than
 * the chain kernel keeps) waits for both to be idle and is done on the spot, so the order of the lines is the file's. */
typedef struct MgQJob
{ struct MgQJob *next; MgChainQ *q; MgChainM *m; int64_t *offsets; char *idBytes; U64 *idOff; int nReads;
  int pinQ, pinOff;                                        /* q / offsets are blocks of the pipe's page-locked pool (slot + 1), not malloc ()ed */
  FmtBuf piece[16]; int nPieces;
} MgQJob;
#define MG_QPIPE_PINS 10
typedef struct { MgQJob *head, *tail; int n; } MgQQueue;
struct MgQueryPipe
{ MgReference *ref; FILE *out; pthread_t thFormat, thWrite; int started;
  pthread_mutex_t mu; pthread_cond_t cv;
  MgQQueue toFormat, toWrite; int pending;                 /* batches anywhere between Push and the last fwrite */
  int closing;
  double msDevice, msFormat, msFormatCpu, msWrite, msWait; int nBatches;      /* (dev timing) */
};

/* page-locked blocks the device halves copy into: kept between calls like the parser's windows (page-locking 10 MB takes 2 ms),
   given back by mgReleaseBuffers ().  A block of at least `bytes` for a job (*slot = its number + 1), or malloc () memory
   (*slot = 0) when the pool has none */
static struct { pthread_mutex_t mu; void *pin[MG_QPIPE_PINS]; size_t cap[MG_QPIPE_PINS]; int busy[MG_QPIPE_PINS]; } gPin = { PTHREAD_MUTEX_INITIALIZER, { 0 }, { 0 }, { 0 } };
static void *pipePinGet (size_t bytes, int *slot)
{
  void *r = 0; *slot = 0;
  pthread_mutex_lock (&gPin.mu);
  int pick = -1;
  for (int i = 0 ; i < MG_QPIPE_PINS ; ++i) if (!gPin.busy[i] && gPin.cap[i] >= bytes && (pick < 0 || gPin.cap[i] < gPin.cap[pick])) pick = i;
  if (pick < 0) for (int i = 0 ; i < MG_QPIPE_PINS ; ++i) if (!gPin.busy[i] && (pick < 0 || gPin.cap[i] < gPin.cap[pick])) pick = i;      /* the smallest free one grows */
  if (pick >= 0) gPin.busy[pick] = 1;
  pthread_mutex_unlock (&gPin.mu);
  if (pick >= 0 && gPin.cap[pick] < bytes)                 /* (busy: nobody else looks at it) */
    { mgPinnedFree (gPin.pin[pick]); gPin.cap[pick] = 0;
      gPin.pin[pick] = mgPinnedAlloc (bytes + bytes / 4);
      if (gPin.pin[pick]) gPin.cap[pick] = bytes + bytes / 4;
      else { pthread_mutex_lock (&gPin.mu); gPin.busy[pick] = 0; pthread_mutex_unlock (&gPin.mu); pick = -1; }
    }
  if (pick >= 0) { r = gPin.pin[pick]; *slot = pick + 1; }
  else { r = malloc (bytes); if (!r) mgFatal ("out of memory"); }
  return r;
}
static void pipePinPut (void *ptr, int slot)
{
  if (!slot) { free (ptr); return; }
  pthread_mutex_lock (&gPin.mu); gPin.busy[slot - 1] = 0; pthread_mutex_unlock (&gPin.mu);
}
void mgQueryReleaseBuffers (void)
{
  pthread_mutex_lock (&gPin.mu);
  for (int i = 0 ; i < MG_QPIPE_PINS ; ++i) if (!gPin.busy[i] && gPin.pin[i]) { mgPinnedFree (gPin.pin[i]); gPin.pin[i] = 0; gPin.cap[i] = 0; }
  pthread_mutex_unlock (&gPin.mu);
  poolFreeAll ();
  mgChainReleaseBuffers ();
}

static void queryJobFree (MgQueryPipe *p, MgQJob *j)
{ pipePinPut (j->q, j->pinQ); pipePinPut (j->offsets, j->pinOff); free (j->m); poolPut (j->idBytes); poolPut (j->idOff);
  for (int t = 0 ; t < j->nPieces ; ++t) poolPut (j->piece[t].buf);
  free (j);
}

/* (all three with p->mu held) */
static void qPut (MgQQueue *q, MgQJob *j) { j->next = 0; if (q->tail) q->tail->next = j; else q->head = j; q->tail = j; ++q->n; }
static MgQJob *qTake (MgQQueue *q) { MgQJob *j = q->head; if (j) { q->head = j->next; if (!q->head) q->tail = 0; --q->n; } return j; }

static void *queryFormatter (void *v)
{
  MgQueryPipe *p = (MgQueryPipe *) v;
  for (;;)
    { pthread_mutex_lock (&p->mu);
      while (!p->toFormat.head && !p->closing) pthread_cond_wait (&p->cv, &p->mu);
      MgQJob *j = qTake (&p->toFormat);
      pthread_mutex_unlock (&p->mu);
      if (!j) break;                                       /* closing, nothing left */
      const char **names = (const char **) poolGet (((size_t) j->nReads + 1) * sizeof (char *));
      mgIdPointers (names, j->idBytes, j->idOff, (size_t) j->nReads);
      queryFormatLines (p->ref, j->q, j->m, j->offsets, j->nReads, names, j->piece, &j->nPieces, &p->msFormat, &p->msFormatCpu);
      poolPut (names);
      pipePinPut (j->q, j->pinQ); pipePinPut (j->offsets, j->pinOff); free (j->m); poolPut (j->idBytes); poolPut (j->idOff);
      j->q = 0; j->m = 0; j->offsets = 0; j->idBytes = 0; j->idOff = 0; j->pinQ = j->pinOff = 0;
      pthread_mutex_lock (&p->mu);
      while (p->toWrite.n >= 2) pthread_cond_wait (&p->cv, &p->mu);
      qPut (&p->toWrite, j);
      pthread_cond_broadcast (&p->cv);
      pthread_mutex_unlock (&p->mu);
    }
  pthread_mutex_lock (&p->mu); p->closing = 2; pthread_cond_broadcast (&p->cv); pthread_mutex_unlock (&p->mu);      /* the writer's turn to finish */
  return 0;
}

static void *queryWriter (void *v)
{
  MgQueryPipe *p = (MgQueryPipe *) v;
  for (;;)
    { pthread_mutex_lock (&p->mu);
      while (!p->toWrite.head && p->closing != 2) pthread_cond_wait (&p->cv, &p->mu);
      MgQJob *j = qTake (&p->toWrite);
      if (j) pthread_cond_broadcast (&p->cv);             /* room in front of the writer */
      pthread_mutex_unlock (&p->mu);
      if (!j) return 0;
      queryWritePieces (j->piece, j->nPieces, p->out, &p->msWrite);
      queryJobFree (p, j);
      pthread_mutex_lock (&p->mu);
      --p->pending;
      pthread_cond_broadcast (&p->cv);
      pthread_mutex_unlock (&p->mu);
    }
}

MgQueryPipe *mgQueryPipeOpen (MgReference *ref, FILE *out)
{
  MgQueryPipe *p = (MgQueryPipe *) calloc (1, sizeof (MgQueryPipe));
  if (!p) mgFatal ("out of memory");
  p->ref = ref; p->out = out;
  pthread_mutex_init (&p->mu, 0); pthread_cond_init (&p->cv, 0);
  if (pthread_create (&p->thFormat, 0, queryFormatter, p) == 0)
    { if (pthread_create (&p->thWrite, 0, queryWriter, p) == 0) p->started = 1;
      else
        { pthread_mutex_lock (&p->mu); p->closing = 1; pthread_cond_broadcast (&p->cv); pthread_mutex_unlock (&p->mu);
          pthread_join (p->thFormat, 0); p->closing = 0;
        }
    }                                                      /* (no threads: Push does everything on the spot) */
  mgChainScratchKeep (1);
  return p;
}

static void queryPipeDrain (MgQueryPipe *p)
{
  pthread_mutex_lock (&p->mu);
  while (p->pending) pthread_cond_wait (&p->cv, &p->mu);
  pthread_mutex_unlock (&p->mu);
}

int mgQueryPipePush (MgQueryPipe *p, const U32 *dPacked, U64 totalBases, const U64 *dReadOffsets, int nReads, const char *idBytes, const U64 *idOff)
{
  if (nReads <= 0) return 0;
  struct timespec c0, c1, c2; clock_gettime (CLOCK_MONOTONIC, &c0);
  const int hostChain = mgKnobs ()->queryHostChain == 1;
  int rc = 1;
  MgQJob *j = 0;
  if (!hostChain && !mgQueryVerbose () && p->started)
    { if (modsetSyncToHost (p->ref->ms, 0)) mgFatal ("modsetSyncToHost");
      j = (MgQJob *) calloc (1, sizeof (MgQJob));
      if (!j) mgFatal ("out of memory");
      j->nReads = nReads;
      j->offsets = (int64_t *) pipePinGet ((size_t) (nReads + 1) * 8, &j->pinOff);
      j->q = (MgChainQ *) pipePinGet ((size_t) nReads * sizeof (MgChainQ), &j->pinQ);
      if (j->pinOff ? mgCopyOutPinned (j->offsets, dReadOffsets, (size_t) (nReads + 1) * 8, 0) : mgMemcpyD2H (j->offsets, dReadOffsets, (size_t) (nReads + 1) * 8, 0)) mgFatal ("D2H");
      rc = mgChainQueryDevice (p->ref, dPacked, totalBases, dReadOffsets, (U32) nReads, j->q, &j->m, MG_QUERY_MAXM, j->pinQ != 0);
      if (rc < 0) mgFatal ("query");
    }
  clock_gettime (CLOCK_MONOTONIC, &c1);
  p->msDevice += mgMsBetween (&c0, &c1); ++p->nBatches;
  if (rc == 1)                                             /* the long way (mg_query.c), on the spot, once the lines before it are out */
    { if (j) queryJobFree (p, j);
      queryPipeDrain (p);
      const char **names = (const char **) malloc (((size_t) nReads + 1) * sizeof (char *));
      if (!names) mgFatal ("out of memory");
      mgIdPointers (names, idBytes, idOff, (size_t) nReads);
      rc = mgQueryProcessDevice (p->ref, dPacked, totalBases, dReadOffsets, nReads, names, p->out);
      free (names);
      return rc;
    }
  /* the ids belong to the parser, which moves on: a copy goes with the job */
  const size_t idLen = (size_t) idOff[nReads - 1] + strlen (idBytes + idOff[nReads - 1]) + 1;
  j->idBytes = (char *) poolGet (idLen); j->idOff = (U64 *) poolGet ((size_t) nReads * 8);
  memcpy (j->idBytes, idBytes, idLen); memcpy (j->idOff, idOff, (size_t) nReads * 8);
  pthread_mutex_lock (&p->mu);
  while (p->toFormat.n >= 2) pthread_cond_wait (&p->cv, &p->mu);
  qPut (&p->toFormat, j); ++p->pending;
  pthread_cond_broadcast (&p->cv);
  pthread_mutex_unlock (&p->mu);
  clock_gettime (CLOCK_MONOTONIC, &c2);
  p->msWait += mgMsBetween (&c1, &c2);
  return 0;
}

void mgQueryPipeClose (MgQueryPipe *p)
{
  if (!p) return;
  struct timespec c0, c1; clock_gettime (CLOCK_MONOTONIC, &c0);
  if (p->started)
    { pthread_mutex_lock (&p->mu); p->closing = 1; pthread_cond_broadcast (&p->cv); pthread_mutex_unlock (&p->mu);
      pthread_join (p->thFormat, 0); pthread_join (p->thWrite, 0);
    }
  clock_gettime (CLOCK_MONOTONIC, &c1);
  mgChainScratchKeep (0);
  if (mgKnobs ()->seedTiming == 1)
    fprintf (stderr, "mgQueryFile: %d batches: device halves %.1f ms, waiting for room in the queue %.1f + %.1f ms at the end; formatter %.1f ms (its threads' CPU time %.1f ms), writer %.1f ms\n",
             p->nBatches, p->msDevice, p->msWait, mgMsBetween (&c0, &c1), p->msFormat, p->msFormatCpu, p->msWrite);
  pthread_mutex_destroy (&p->mu); pthread_cond_destroy (&p->cv);
  free (p);
}
