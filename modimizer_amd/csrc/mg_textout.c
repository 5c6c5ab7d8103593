/* mg_textout.c — modutils -P / -d: the reports' writer.
 * The reports' text is made on the device (mg_report.hip); what is left here is moving it out: a chunk's bytes are copied into
 * page-locked blocks of up to MG_TOUT_PIECE bytes on the caller's thread, and a writer thread fwrite()s the blocks in the order they
 * were filled while the device formats the next chunk.  MG_TOUT_BLOCKS blocks: the caller waits for one to be free.
 */
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include "modgpu.h"
#include "mg_internal.h"

#define MG_TOUT_BLOCKS 4
#define MG_TOUT_PIECE ((size_t) 32 << 20)
struct MgTextOut
{ FILE *out; pthread_t th; int started, closing, err;
  pthread_mutex_t mu; pthread_cond_t cv;
  char *blk[MG_TOUT_BLOCKS]; size_t cap[MG_TOUT_BLOCKS], len[MG_TOUT_BLOCKS]; int pinned[MG_TOUT_BLOCKS], busy[MG_TOUT_BLOCKS];
  int queue[MG_TOUT_BLOCKS], qHead, qN;                    /* blocks filled and not yet written, in order */
  double msCopy, msWrite; unsigned long long bytes;        /* (MODGPU_SEED_TIMING=1 prints them at the close) */
};

static void *textOutWriter (void *v)
{
  MgTextOut *w = (MgTextOut *) v;
  for (;;)
    { pthread_mutex_lock (&w->mu);
      while (!w->qN && !w->closing) pthread_cond_wait (&w->cv, &w->mu);
      if (!w->qN) { pthread_mutex_unlock (&w->mu); return 0; }
      const int b = w->queue[w->qHead];
      pthread_mutex_unlock (&w->mu);
      struct timespec t0, t1; clock_gettime (CLOCK_MONOTONIC, &t0);
      const int bad = fwrite (w->blk[b], 1, w->len[b], w->out) != w->len[b];
      clock_gettime (CLOCK_MONOTONIC, &t1);
      pthread_mutex_lock (&w->mu);
      w->msWrite += mgMsBetween (&t0, &t1); if (bad) w->err = 1;
      w->qHead = (w->qHead + 1) % MG_TOUT_BLOCKS; --w->qN; w->busy[b] = 0;
      pthread_cond_broadcast (&w->cv);
      pthread_mutex_unlock (&w->mu);
    }
}

MgTextOut *mgTextOutOpen (FILE *out)
{
  MgTextOut *w = (MgTextOut *) calloc (1, sizeof (MgTextOut));
  if (!w) mgFatal ("out of memory");
  w->out = out;
  pthread_mutex_init (&w->mu, 0); pthread_cond_init (&w->cv, 0);
  w->started = pthread_create (&w->th, 0, textOutWriter, w) == 0;     /* (no thread: every block is written on the spot) */
  return w;
}

int mgTextOutFromDevice (MgTextOut *w, const void *dSrc, size_t bytes)
{
  for (size_t off = 0 ; off < bytes ; )
    { const size_t piece = bytes - off < MG_TOUT_PIECE ? bytes - off : MG_TOUT_PIECE;
      int b = -1;
      pthread_mutex_lock (&w->mu);
      for (;;)
        { for (int i = 0 ; i < MG_TOUT_BLOCKS ; ++i) if (!w->busy[i] && (b < 0 || (w->cap[b] < piece && w->cap[i] > w->cap[b]))) b = i;
          if (b >= 0) break;
          pthread_cond_wait (&w->cv, &w->mu);
        }
      w->busy[b] = 1;
      pthread_mutex_unlock (&w->mu);
      if (w->cap[b] < piece)                              /* (busy: the writer does not look at it) */
        { if (w->pinned[b]) mgPinnedFree (w->blk[b]); else free (w->blk[b]);
          size_t want = bytes - off > MG_TOUT_PIECE ? MG_TOUT_PIECE : ((piece + (1 << 20) - 1) & ~(size_t) ((1 << 20) - 1));
          w->blk[b] = (char *) mgPinnedAlloc (want); w->pinned[b] = w->blk[b] != 0;
          if (!w->blk[b]) w->blk[b] = (char *) malloc (want);
          if (!w->blk[b]) mgFatal ("out of memory");
          w->cap[b] = want;
        }
      struct timespec t0, t1; clock_gettime (CLOCK_MONOTONIC, &t0);
      if (mgMemcpyD2H (w->blk[b], (const char *) dSrc + off, piece, 0))
        { pthread_mutex_lock (&w->mu); w->busy[b] = 0; pthread_mutex_unlock (&w->mu); return -1; }
      clock_gettime (CLOCK_MONOTONIC, &t1);
      w->msCopy += mgMsBetween (&t0, &t1); w->bytes += piece;
      w->len[b] = piece;
      off += piece;
      if (!w->started)
        { struct timespec t2; if (fwrite (w->blk[b], 1, piece, w->out) != piece) w->err = 1;
          clock_gettime (CLOCK_MONOTONIC, &t2); w->msWrite += mgMsBetween (&t1, &t2);
          w->busy[b] = 0;
          continue;
        }
      pthread_mutex_lock (&w->mu);
      w->queue[(w->qHead + w->qN) % MG_TOUT_BLOCKS] = b; ++w->qN;
      pthread_cond_broadcast (&w->cv);
      pthread_mutex_unlock (&w->mu);
    }
  return 0;
}

int mgTextOutClose (MgTextOut *w)
{
  if (!w) return 0;
  struct timespec t0, t1; clock_gettime (CLOCK_MONOTONIC, &t0);
  if (w->started)
    { pthread_mutex_lock (&w->mu); w->closing = 1; pthread_cond_broadcast (&w->cv); pthread_mutex_unlock (&w->mu);
      pthread_join (w->th, 0);
    }
  clock_gettime (CLOCK_MONOTONIC, &t1);
  if (mgKnobs ()->seedTiming == 1)
    fprintf (stderr, "mgTextOut: %llu bytes, device -> page-locked copies %.1f ms, writer %.1f ms (%.0f MB/s), wait at the close %.1f ms\n",
             w->bytes, w->msCopy, w->msWrite, w->msWrite > 0 ? w->bytes / w->msWrite * 1e-3 : 0.0, mgMsBetween (&t0, &t1));
  const int err = w->err;
  for (int i = 0 ; i < MG_TOUT_BLOCKS ; ++i) { if (w->pinned[i]) mgPinnedFree (w->blk[i]); else free (w->blk[i]); }
  pthread_mutex_destroy (&w->mu); pthread_cond_destroy (&w->cv);
  free (w);
  return err ? -1 : 0;
}
