/* mg_hostbatch.hip — the entry points that take host bytes and return host arrays (layer 2 of include/modgpu.h): the threaded
 * pack-and-upload stage (mgUploadPack), the scan and minimizer batches, mgAddSequenceBatch with its grow-only device buffers, the
 * depth histogram as text, and the per-read iterator facade that mg_host.c's modRCiterator / minimizer iterator replay.
 */
#include <pthread.h>
#include <unistd.h>
#include <immintrin.h>
#include <atomic>
#include <thread>
#include <vector>
#include "mg_api_int.h"

#define MG_MAXDEV 128            /* (an 8-GPU node in its 8-partition mode shows 64 devices) */
/* what is kept per device between calls (byDev[MG_MAXDEV], each with its lock) given back: drop (x) on the device it lives on wherever
   holds (x), the caller's device current again afterwards */
template <class T, class Holds, class Drop> static void mgDropOnEachDevice (T *byDev, Holds holds, Drop drop)
{
  int before = -1; if (hipGetDevice (&before) != hipSuccess) { (void) hipGetLastError (); before = -1; }
  for (int dev = 0 ; dev < MG_MAXDEV ; ++dev)
    { T &x = byDev[dev];
      std::lock_guard<std::mutex> g (x.lock);
      if (!holds (x)) continue;
      (void) hipSetDevice (dev);
      drop (x);
    }
  if (before >= 0) (void) hipSetDevice (before);
}

/* Host bytes (one base per byte) -> 2-bit packed words in HBM.  The bytes are packed ON THE HOST by a team of
 * threads (mg_pack.c: 128 bases per AVX2 step) into two pinned staging buffers, piece by piece, and each piece goes
 * across PCIe as packed words (a quarter of the bytes) with an asynchronous copy that overlaps the packing of the
 * next piece.  (Before: the bytes crossed as they were and were packed on the device: 1 byte per base on the link.) */
extern "C" void mgPackWords (const char *bases, U64 nBases, U32 *words);      /* mg_pack.c */
#define MG_UP_PIECE ((U64) 128 << 20)                 /* bases per piece (a multiple of 16): 32 MiB of packed words */
static struct MgUpStage { U32 *pin[2] = { 0, 0 }; hipEvent_t done[2]; bool ready = false; std::mutex lock; } gUps[MG_MAXDEV];   /* by device (the events belong to one): host threads that drive several GPUs do not take turns on one stage, nor re-make it at every switch */

void mgUploadRelease (void)
{
  auto drop = [] (MgUpStage &u)
    { for (int i = 0 ; i < 2 ; ++i) { if (u.ready) (void) hipEventDestroy (u.done[i]); if (u.pin[i]) (void) hipHostFree (u.pin[i]); u.pin[i] = 0; }
      u.ready = false;
    };
  mgDropOnEachDevice (gUps, [] (MgUpStage &u) { return u.ready || u.pin[0] || u.pin[1]; }, drop);
}

static int mgHostThreads (void)
{
  static int n = 0;
  if (n) return n;
  const long kv = mgKnobs ()->packThreads;
  long v = kv != MG_KNOB_UNSET ? kv : 0;
  if (v <= 0) v = mgCpuBudget ();                                      /* (a cgroup CPU quota caps what threads can get) */
  if (kv == MG_KNOB_UNSET) v = v / 2;                                   /* measured (16-CPU quota): 8 packers keep the link busy, 16 starve the thread that issues the copies */
  if (v < 1) v = 1;
  if (v > 16) v = 16;
  return n = (int) v;
}

extern "C" MgStatus mgUploadPack (const char *bases, U64 nBases, U32 *dPacked, void *stream)
{
  MgStatus s = mgEnsureDevice (); if (s) return s;
  hipStream_t st = (hipStream_t) stream;
  if (!nBases) { MG_HIP (hipMemsetAsync (dPacked, 0, mgPackedWords (0) * 4, st)); return MG_OK; }
  int curDev = 0; MG_HIP (hipGetDevice (&curDev));
  if (curDev < 0 || curDev >= MG_MAXDEV) { mgSetError ("mgUploadPack: device number beyond %d", MG_MAXDEV - 1); return MG_ERR_ARG; }
  MgUpStage &gUp = gUps[curDev];
  std::lock_guard<std::mutex> g (gUp.lock);
  if (!gUp.ready)
    { for (int i = 0 ; i < 2 ; ++i)
        { if (!gUp.pin[i]) MG_HIP (hipHostMalloc ((void **) &gUp.pin[i], (MG_UP_PIECE / 16 + MG_PACK_PAD) * 4, hipHostMallocPortable));
          MG_HIP (hipEventCreateWithFlags (&gUp.done[i], hipEventDisableTiming));
        }
      gUp.ready = true;
    }
  const U64 nPieces = (nBases + MG_UP_PIECE - 1) / MG_UP_PIECE;
  int T = mgHostThreads ();
  if (nBases < ((U64) 1 << 20)) T = 1;
  pthread_barrier_t bar;
  /* every thread packs its share of every piece; thread 0 also waits for the staging buffer to be free before a
     piece and sends the piece off after it */
  volatile int failed = 0;
  auto work = [&] (int t)
    { for (U64 p = 0 ; p < nPieces ; ++p)
        { const U64 off = p * MG_UP_PIECE, len = nBases - off < MG_UP_PIECE ? nBases - off : MG_UP_PIECE;
          U32 *buf = gUp.pin[p & 1];
          if (t == 0 && p >= 2 && hipEventSynchronize (gUp.done[p & 1]) != hipSuccess) failed = 1;    /* the copy that last read this buffer */
          pthread_barrier_wait (&bar);
          const U64 words = (len + 15) / 16, per = ((words + T - 1) / T + 7) & ~(U64) 7;               /* whole words per thread, a multiple of 8 */
          const U64 w0 = per * (U64) t < words ? per * (U64) t : words, w1 = w0 + per < words ? w0 + per : words;
          if (w1 > w0)
            { const U64 b0 = w0 * 16, b1 = w1 * 16 < len ? w1 * 16 : len;
              mgPackWords (bases + off + b0, b1 - b0, buf + w0);
            }
          pthread_barrier_wait (&bar);
          if (t == 0)
            { U64 n = words;
              if (p + 1 == nPieces) { for (int j = 0 ; j < MG_PACK_PAD ; ++j) buf[words + j] = 0; n += MG_PACK_PAD; }   /* the pad words after the stream */
              if (hipMemcpyAsync (dPacked + off / 16, buf, n * 4, hipMemcpyHostToDevice, st) != hipSuccess
                  || hipEventRecord (gUp.done[p & 1], st) != hipSuccess) failed = 1;
            }
        }
    };
  /* the helpers are started first and held at a gate: if the system will not give T threads, those that did start are
     sent home and the caller packs alone (a thread constructor that throws must not leave threads at the barrier) */
  std::vector<std::thread> th;
  std::atomic<int> gate (0);
  auto helper = [&] (int t) { int v; while (!(v = gate.load (std::memory_order_acquire))) std::this_thread::yield (); if (v > 0) work (t); };
  try { for (int t = 1 ; t < T ; ++t) th.emplace_back (helper, t); }
  catch (...) { gate.store (-1, std::memory_order_release); for (auto &x : th) x.join (); th.clear (); T = 1; }
  pthread_barrier_init (&bar, 0, (unsigned) T);
  gate.store (1, std::memory_order_release);
  work (0);
  for (auto &x : th) x.join ();
  pthread_barrier_destroy (&bar);
  if (failed) return mgHipFail (hipGetLastError (), "mgUploadPack");
  MG_HIP (hipStreamSynchronize (st));
  return MG_OK;
}

/* ---------------------------------------------------------------------------------------- */
/* scan                                                                                       */

extern "C" MgStatus seqhashScanBatchDevice (const Seqhash *sh, const U32 *dPacked, U64 totalBases,
                                            const U64 *dReadOffsets, U32 nReads,
                                            U64 *dKmer, U32 *dPosF, U32 *dReadId, U64 capacity,
                                            U64 *dCount, void *dWork, void *stream)
{
  MgStatus s = mgEnsureDevice (); if (s) return s;
  if ((s = mgCheckHasher (sh))) return s;
  if (!dCount || (totalBases && (!dPacked || !dReadOffsets || !dWork)))
    { mgSetError ("seqhashScanBatchDevice: null argument"); return MG_ERR_ARG; }
  return mgLaunchScan (mgMakeParams (sh), dPacked, totalBases, dReadOffsets, nReads,
                       dKmer, dPosF, dReadId, capacity, dCount, dWork, (hipStream_t) stream);
}

U64 mgSurvivorGuess (const Seqhash *sh, U64 totalBases)
{
  U64 g = totalBases / (U64) sh->w;
  g += g / 4 + (1 << 16);
  return g < totalBases ? g : totalBases;
}

/* a host batch's read offsets: 0 when they can be used, else -1 with who's error */
static int mgCheckReadOffsets (const char *who, const int64_t *readOffsets, int nReads)
{ if (nReads < 0 || (nReads && (!readOffsets || readOffsets[0] != 0))) { mgSetError ("%s: bad read offsets", who); return -1; } return 0; }
/* n entries of pos | isF << 31 as the reference's callers take them: malloc ()ed pos[] and isF[], each only where wanted */
static void mgSplitPosF (const U32 *hP, int64_t n, int **posOut, bool **isFOut)
{
  if (posOut) { int *p = (int *) malloc ((n + 1) * sizeof (int)); for (int64_t i = 0 ; i < n ; ++i) p[i] = (int) (hP[i] & MG_POS_MASK); *posOut = p; }
  if (isFOut) { bool *f = (bool *) malloc ((n + 1) * sizeof (bool)); for (int64_t i = 0 ; i < n ; ++i) f[i] = (hP[i] & MG_FWD_BIT) != 0; *isFOut = f; }
}

extern "C" int64_t seqhashScanBatch (const Seqhash *sh, const char *bases, const int64_t *readOffsets, int nReads,
                                     U64 **kmerOut, int **posOut, bool **isFOut, int64_t **survStartOut)
{
  if (mgEnsureDevice () || mgCheckHasher (sh) || mgCheckReadOffsets ("seqhashScanBatch", readOffsets, nReads)) return -1;
  U64 total = nReads ? (U64) readOffsets[nReads] : 0;
  size_t nw = mgPackedWords (total);
  U64 cap = mgSurvivorGuess (sh, total);
  MgArena ar;
  int64_t result = -1;
  U64 *hK = 0; U32 *hP = 0, *hR = 0;
  for (int attempt = 0 ; attempt < 3 ; ++attempt)
    { size_t need = mgAl256 (nw * 4) + mgAl256 (((size_t) nReads + 1) * 8) + mgAl256 (cap * 8) + 2 * mgAl256 (cap * 4)
                    + mgAl256 (mgScanWorkBytes (total, (U32) nReads, cap)) + 4096;
      if (ar.reserve (need)) break;
      ar.reset ();
      U32 *dP = (U32 *) ar.take (nw * 4);
      U64 *dOff = (U64 *) ar.take (((size_t) nReads + 1) * 8);
      U64 *dK = (U64 *) ar.take (cap * 8);
      U32 *dPos = (U32 *) ar.take (cap * 4);
      U32 *dRid = (U32 *) ar.take (cap * 4);
      void *dWork = ar.take (mgScanWorkBytes (total, (U32) nReads, cap));
      U64 *dCount = (U64 *) ar.take (8 * MG_COUNT_WORDS);
      if (mgUploadPack (bases, total, dP, 0)) break;
      if (nReads && hipMemcpy (dOff, readOffsets, ((size_t) nReads + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) break;
      if (seqhashScanBatchDevice (sh, dP, total, dOff, (U32) nReads, dK, dPos, dRid, cap, dCount, dWork, 0)) break;
      U64 cnt[MG_COUNT_WORDS], n;
      if (hipMemcpy (cnt, dCount, sizeof (cnt), hipMemcpyDeviceToHost) != hipSuccess) break;
      const U64 again = mgScanRetryCap (cnt, cap, &n);
      if (again) { cap = again; continue; }
      hK = (U64 *) malloc ((n + 1) * 8); hP = (U32 *) malloc ((n + 1) * 4); hR = (U32 *) malloc ((n + 1) * 4);
      if (n)
        { if (hipMemcpy (hK, dK, n * 8, hipMemcpyDeviceToHost) != hipSuccess) break;
          if (hipMemcpy (hP, dPos, n * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
          if (hipMemcpy (hR, dRid, n * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
        }
      result = (int64_t) n;
      break;
    }
  ar.release ();
  if (result < 0)
    { if (!mgLastError ()[0]) mgSetError ("seqhashScanBatch: device failure");
      free (hK); free (hP); free (hR); return -1;
    }
  int64_t n = result;
  mgSplitPosF (hP, n, posOut, isFOut);
  if (survStartOut)
    { int64_t *st = (int64_t *) malloc (((size_t) nReads + 1) * sizeof (int64_t));
      int64_t i = 0;
      for (int r = 0 ; r <= nReads ; ++r) { while (i < n && (int64_t) hR[i] < r) ++i; st[r] = i; }
      *survStartOut = st;
    }
  if (kmerOut) *kmerOut = hK; else free (hK);
  free (hP); free (hR);
  return n;
}

/* ---------------------------------------------------------------------------------------- */
/* minimizers (seqhash.c:83-152) */

extern "C" MgStatus seqhashMinimizerBatchDevice (const Seqhash *sh, const U32 *dPacked, U64 totalBases,
                                                 const U64 *dReadOffsets, U32 nReads,
                                                 U64 *dHash, U32 *dPosF, U64 *dReadStart, U64 capacity,
                                                 U64 *nOut, void *stream)
{
  MgStatus s = mgEnsureDevice (); if (s) return s;
  if ((s = mgCheckHasher (sh))) return s;
  (void) totalBases;
  U64 total = 0;
  s = mgLaunchMinimizers (mgMakeParams (sh), (U32) sh->w, dPacked, dReadOffsets, nReads, dHash, dPosF, dReadStart,
                          capacity, &total, (hipStream_t) stream);
  if (nOut) *nOut = total;
  return s;
}

/* host buffers in, host arrays out; *startOut[r] .. [r+1] are read r's minimizers.  Returns their number, -1 on error. */
static int64_t mgMinimizersHost (const Seqhash *sh, const char *bases, const int64_t *readOffsets, int nReads,
                                 U64 **hashOut, U32 **posFOut, int64_t **startOut)
{
  if (mgEnsureDevice () || mgCheckHasher (sh) || mgCheckReadOffsets ("minimizer batch", readOffsets, nReads)) return -1;
  const U64 total = nReads ? (U64) readOffsets[nReads] : 0;
  const size_t nw = mgPackedWords (total);
  U64 cap = total / ((U64) sh->w / 2 + 1) + total / 8 + (U64) nReads + 1024;
  int64_t result = -1;
  U64 *hH = 0; U32 *hP = 0; int64_t *hS = 0;
  MgArena ar;
  for (int attempt = 0 ; attempt < 2 ; ++attempt)
    { size_t need = mgAl256 (nw * 4) + 2 * mgAl256 (((size_t) nReads + 2) * 8) + mgAl256 (cap * 8) + mgAl256 (cap * 4) + 4096;
      if (ar.reserve (need)) break;
      ar.reset ();
      U32 *dP = (U32 *) ar.take (nw * 4);
      U64 *dOff = (U64 *) ar.take (((size_t) nReads + 2) * 8);
      U64 *dStart = (U64 *) ar.take (((size_t) nReads + 2) * 8);
      U64 *dH = (U64 *) ar.take (cap * 8);
      U32 *dQ = (U32 *) ar.take (cap * 4);
      if (mgUploadPack (bases, total, dP, 0)) break;
      if (nReads && hipMemcpy (dOff, readOffsets, ((size_t) nReads + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) break;
      U64 n = 0;
      MgStatus s = seqhashMinimizerBatchDevice (sh, dP, total, dOff, (U32) nReads, dH, dQ, dStart, cap, &n, 0);
      if (s == MG_ERR_CAPACITY && attempt == 0) { cap = n; continue; }
      if (s) break;
      hH = (U64 *) malloc ((n + 1) * 8); hP = (U32 *) malloc ((n + 1) * 4); hS = (int64_t *) malloc (((size_t) nReads + 1) * 8);
      if (hipStreamSynchronize (0) != hipSuccess) break;
      if (n && (hipMemcpy (hH, dH, n * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy (hP, dQ, n * 4, hipMemcpyDeviceToHost) != hipSuccess)) break;
      if (hipMemcpy (hS, dStart, ((size_t) nReads + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) break;
      result = (int64_t) n;
      break;
    }
  ar.release ();
  if (result < 0)
    { if (!mgLastError ()[0]) mgSetError ("minimizer batch: device failure");
      free (hH); free (hP); free (hS); return -1;
    }
  *hashOut = hH; *posFOut = hP; *startOut = hS;
  return result;
}

extern "C" int64_t seqhashMinimizerBatch (const Seqhash *sh, const char *bases, const int64_t *readOffsets, int nReads,
                                          U64 **hashOut, int **posOut, bool **isFOut, int64_t **startOut)
{
  U64 *hH = 0; U32 *hP = 0; int64_t *hS = 0;
  int64_t n = mgMinimizersHost (sh, bases, readOffsets, nReads, &hH, &hP, &hS);
  if (n < 0) return -1;
  mgSplitPosF (hP, n, posOut, isFOut);
  if (hashOut) *hashOut = hH; else free (hH);
  if (startOut) *startOut = hS; else free (hS);
  free (hP);
  return n;
}

/* one read for the iterator facade: *rec = malloc()ed {n hashes (U64), n posF (U32)} */
extern "C" int mgIterMinScan (Seqhash *sh, const char *s, int len, U64 **rec, U64 *nOut)
{
  *rec = 0; *nOut = 0;
  if (len < sh->k) return mgEnsureDevice () ? -1 : 0;
  int64_t off[2] = { 0, len };
  U64 *hH = 0; U32 *hP = 0; int64_t *hS = 0;
  int64_t n = mgMinimizersHost (sh, s, off, 1, &hH, &hP, &hS);
  if (n < 0) return -1;
  U64 *blk = (U64 *) malloc ((size_t) n * 12 + 16);
  memcpy (blk, hH, (size_t) n * 8);
  memcpy (blk + n, hP, (size_t) n * 4);
  free (hH); free (hP); free (hS);
  *rec = blk; *nOut = (U64) n;
  return 0;
}

/* ---------------------------------------------------------------------------------------- */
/* host-buffer mirrors of the reference callers' loops                                        */

/* grow-only device buffers for the host-buffer entry points (a hipMalloc + hipFree of a gigabyte per call costs
 * milliseconds): the packed reads and their offsets of the batch in flight */
static struct MgHostBatchBufs { MgDevBuf<U32> dP; MgDevBuf<U64> dOff; std::mutex lock; } gHbs[MG_MAXDEV];   /* by device */
extern "C" void mgHostBatchRelease (void)
{
  mgDropOnEachDevice (gHbs, [] (MgHostBatchBufs &b) { return b.dP.p || b.dOff.p; }, [] (MgHostBatchBufs &b) { b.dP.drop (); b.dOff.drop (); });
}

extern "C" int64_t mgAddSequenceBatch (Modset *ms, const char *bases, const int64_t *readOffsets, int nReads)
{
  if (mgEnsureDevice ()) return -1;
  if (nReads <= 0) return 0;
  const int timing = mgKnobs ()->uploadTiming == 1;   /* dev */
  int curDev = 0; if (hipGetDevice (&curDev) != hipSuccess) { mgSetError ("mgAddSequenceBatch: no current device"); return -1; }
  if (curDev < 0 || curDev >= MG_MAXDEV) { mgSetError ("mgAddSequenceBatch: device number beyond %d", MG_MAXDEV - 1); return -1; }
  MgHostBatchBufs &gHb = gHbs[curDev];
  std::lock_guard<std::mutex> g (gHb.lock);            /* the buffers of this device: one batch at a time through them; a thread on another GPU has that GPU's */
  U64 total = (U64) readOffsets[nReads];
  size_t nw = mgPackedWords (total);
  if (gHb.dP.reserve (nw, nw + nw / 8, "mgAddSequenceBatch") || gHb.dOff.reserve ((size_t) nReads + 1, ((size_t) nReads + 1) * 2, "mgAddSequenceBatch")) return -1;
  int64_t res = -1;
  const double t0 = mgNowS ();
  if (hipMemcpyAsync (gHb.dOff.p, readOffsets, ((size_t) nReads + 1) * 8, hipMemcpyHostToDevice, 0) == hipSuccess
      && mgUploadPack (bases, total, gHb.dP.p, 0) == MG_OK)
    { const double t1 = mgNowS ();
      U64 nHash = 0;
      if (mgAddReadsDevice (ms, gHb.dP.p, total, gHb.dOff.p, (U32) nReads, &nHash, 0) == MG_OK) res = (int64_t) nHash;
      if (timing) fprintf (stderr, "mgAddSequenceBatch: %.3f Gbp  pack+upload %.2f ms  scan+build %.2f ms\n", total / 1e9, (t1 - t0) * 1e3, (mgNowS () - t1) * 1e3);
    }
  else mgSetError ("mgAddSequenceBatch: copy to the device failed");
  return res;
}

extern "C" void mgDepthHistogram (Modset *ms, FILE *f)
{
  U64 *hist = (U64 *) calloc (65536, sizeof (U64));
  MgDev *d = mgDevLookup (ms);
  bool done = false;
  if (d)
    { MgDevScratch scratch ("depth histogram");
      U64 *dHist;
      if (!scratch.get (&dHist, 65536) && hipMemset (dHist, 0, 65536 * 8) == hipSuccess && modsetDepthHistogramDevice (ms, dHist, 0) == MG_OK
          && hipMemcpy (hist, dHist, 65536 * 8, hipMemcpyDeviceToHost) == hipSuccess) done = true;
      if (!done) { fprintf (stderr, "FATAL ERROR: depth histogram on device failed: %s\n", mgLastError ()); exit (-1); }
    }
  else
    for (U32 i = 1 ; i <= ms->max ; ++i) ++hist[ms->depth[i]];      /* host-only modset: nothing on the device */
  for (U32 b = 0 ; b < 65536 ; ++b)
    if (hist[b]) fprintf (f, "DP\t%u\t%u\n", b, (U32) hist[b]);       /* modutils.c:61 */
  free (hist);
}

/* ---------------------------------------------------------------------------------------- */
/* per-read iterator facade: one GPU scan per modRCiterator call, replayed by modRCnext       */

/* The reference's callers scan read by read (modutils.c:19-31, modmap.c:197-206): modRCiterator, modRCnext until false,
 * destroy.  One call here = pack the read into a pinned host buffer the GPU reads in place, ONE kernel launch
 * (mgIterScanKernel: scan + ordered concatenation + completion flag), the replay block {n, k-mers, pos|isF} written by the
 * kernel straight into pinned host memory, the host polling the flag: no host-to-device or device-to-host copy call and
 * no stream wait on the way.  Reads longer than mgIterMaxBases () take the batch scan with the block copied back.
 * The scratch is per host thread and per device. */
static bool gRuntimeAlive = true;                          /* false once the library is being unloaded: thread-local destructors that run after that leave HIP alone */
__attribute__ ((destructor)) static void mgRuntimeDown (void) { gRuntimeAlive = false; }
static bool mgRuntimeAlive (void) { return gRuntimeAlive; }
struct MgIterScratch {
  int dev = -1; hipStream_t st = 0;
  char *hIn = 0; char *dIn = 0; size_t inBytes = 0;          /* pinned: {0, len} (2 x U64), then the packed words */
  U64 *hOut = 0; U64 *dOut = 0; size_t outEntries = 0;       /* pinned: the replay block */
  U64 *hFlag = 0; U64 *dFlag = 0; U64 seq = 0;               /* pinned: the kernel's completion flag */
  U64 *dSegK = 0; U32 *dSegP = 0;                            /* device: the workers' segments */
  /* the long-read path */
  MgDevBuf<U32> dPacked; MgDevBuf<U64> dKmer; MgDevBuf<U32> dPosF; MgDevBuf<char> dWork;      /* (dKmer and dPosF grow together) */
  U64 *dOff = 0; U64 *dCount = 0;
  U32 *hPacked = 0; size_t hWordsCap = 0;
  ~MgIterScratch () { if (dev >= 0 && mgRuntimeAlive ()) release (); }      /* a host thread that ends gives its pinned buffers and its stream back */
  void release ()
  { if (st) (void) hipStreamSynchronize (st);              /* no kernel of this scratch is still writing into what is freed */
    if (hIn) (void) hipHostFree (hIn);
    if (hOut) (void) hipHostFree (hOut);
    if (hFlag) (void) hipHostFree (hFlag);
    (void) hipFree (dSegK); (void) hipFree (dSegP); (void) hipFree (dOff); (void) hipFree (dCount);
    dPacked.drop (); dKmer.drop (); dPosF.drop (); dWork.drop ();
    if (st) (void) hipStreamDestroy (st);
    free (hPacked);
    *this = MgIterScratch ();
  }
};
static thread_local MgIterScratch gIt;

static int mgIterPinned (void **h, void **d, size_t bytes)
{
  if (hipHostMalloc (h, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return -1;
  if (hipHostGetDevicePointer (d, *h, 0) != hipSuccess) return -1;
  return 0;
}

/* the scratch for the calling thread on the current device */
static int mgIterPrepare (MgIterScratch &g)
{
  int dev = 0;
  if (hipGetDevice (&dev) != hipSuccess) return -1;
  if (g.dev == dev) return 0;
  if (g.dev >= 0) g.release ();                        /* the thread moved to another GPU (mgSetDevice) */
  g.inBytes = 16 + mgPackedWords (mgIterMaxBases ()) * 4;
  if (hipStreamCreateWithFlags (&g.st, hipStreamNonBlocking) != hipSuccess) return -1;
  if (mgIterPinned ((void **) &g.hIn, (void **) &g.dIn, g.inBytes)) return -1;
  if (mgIterPinned ((void **) &g.hFlag, (void **) &g.dFlag, 64)) return -1;
  g.hFlag[0] = 0;
  if (hipMalloc ((void **) &g.dSegK, mgIterSegEntries () * 8) != hipSuccess || hipMalloc ((void **) &g.dSegP, mgIterSegEntries () * 4) != hipSuccess) return -1;
  g.dev = dev;
  return 0;
}

static int mgIterOutReserve (MgIterScratch &g, size_t entries)
{
  if (entries <= g.outEntries) return 0;
  if (g.hOut) { (void) hipStreamSynchronize (g.st); (void) hipHostFree (g.hOut); g.hOut = 0; g.outEntries = 0; }
  const size_t want = entries + entries / 4 + 4096;
  if (mgIterPinned ((void **) &g.hOut, (void **) &g.dOut, (want + 2) * 12)) return -1;
  g.outEntries = want;
  return 0;
}

/* reads beyond the one-launch kernel's reach: the batch scan, the block copied back */
static int mgIterScanLong (MgIterScratch &g, Seqhash *sh, const char *s, U64 total, U64 **blkOut)
{
  size_t nw = mgPackedWords (total);
  if (nw > g.hWordsCap) { free (g.hPacked); g.hPacked = (U32 *) malloc (2 * nw * 4); g.hWordsCap = 2 * nw; }
  mgPackHost (s, total, g.hPacked);
  if (!g.dOff) { if (hipMalloc ((void **) &g.dOff, 16) != hipSuccess || hipMalloc ((void **) &g.dCount, 8 * MG_COUNT_WORDS) != hipSuccess) return -1; }
  const char *const what = "iterator scan of a long read";
  if (g.dPacked.reserve (nw, 2 * nw, what)) return -1;
  U64 cap = mgSurvivorGuess (sh, total);
  MgHashParams p = mgMakeParams (sh);
  U64 off[2] = { 0, total };
  for (int attempt = 0 ; attempt < 3 ; ++attempt)
    { if (g.dKmer.reserve (cap, 2 * cap, what) || g.dPosF.reserve (cap, 2 * cap, what)) return -1;
      const U64 survCap = std::min (g.dKmer.cap, g.dPosF.cap);
      const size_t wb = mgScanWorkBytes (total, 1, survCap);
      if (g.dWork.reserve (wb, 2 * wb, what)) return -1;
      if (hipMemcpyAsync (g.dPacked.p, g.hPacked, nw * 4, hipMemcpyHostToDevice, g.st) != hipSuccess) return -1;
      if (hipMemcpyAsync (g.dOff, off, 16, hipMemcpyHostToDevice, g.st) != hipSuccess) return -1;
      if (mgLaunchScan (p, g.dPacked.p, total, g.dOff, 1, g.dKmer.p, g.dPosF.p, 0, survCap, g.dCount, g.dWork.p, g.st)) return -1;
      U64 c[MG_COUNT_WORDS], n;
      if (hipMemcpyAsync (c, g.dCount, sizeof (c), hipMemcpyDeviceToHost, g.st) != hipSuccess || hipStreamSynchronize (g.st) != hipSuccess) return -1;
      if ((cap = mgScanRetryCap (c, survCap, &n))) continue;
      U64 *blk = (U64 *) malloc ((size_t) (n + 1) * 8 + (size_t) n * 4 + 8);
      if (!blk) return -1;
      blk[0] = n;
      if (n && (hipMemcpyAsync (blk + 1, g.dKmer.p, n * 8, hipMemcpyDeviceToHost, g.st) != hipSuccess
                || hipMemcpyAsync (blk + 1 + n, g.dPosF.p, n * 4, hipMemcpyDeviceToHost, g.st) != hipSuccess
                || hipStreamSynchronize (g.st) != hipSuccess)) { free (blk); return -1; }
      *blkOut = blk;
      return 0;
    }
  return -1;
}

/* returns 0 on success; *blkOut is the malloc()ed replay block {n, n k-mers (U64), n pos | isF << 31 (U32)} -- what the
   iterator's hashBuf points to (the reference's callers free () it: seqhash.h:54-55) */
extern "C" int mgIterScan (Seqhash *sh, const char *s, int len, U64 **blkOut)
{
  *blkOut = 0;
  if (mgEnsureDevice ()) return -1;
  if (len < sh->k)
    { U64 *blk = (U64 *) malloc (16); if (!blk) return -1;
      blk[0] = 0; *blkOut = blk; return 0;
    }
  MgIterScratch &g = gIt;
  if (mgIterPrepare (g)) { if (!mgLastError ()[0]) mgSetError ("iterator scratch: %s", hipGetErrorString (hipGetLastError ())); return -1; }
  const U64 total = (U64) len;
  if (total > mgIterMaxBases ()) return mgIterScanLong (g, sh, s, total, blkOut);
  U64 *hdr = (U64 *) g.hIn; hdr[0] = 0; hdr[1] = total;
  mgPackHost (s, total, (U32 *) (g.hIn + 16));
  U64 want = total / (U64) sh->w + total / (4 * (U64) sh->w) + 256;      /* expected modimizers, a quarter more; the kernel says so if it was not enough */
  const MgHashParams p = mgMakeParams (sh);
  for (int attempt = 0 ; attempt < 2 ; ++attempt)
    { if (mgIterOutReserve (g, want)) { mgSetError ("iterator scratch: pinned allocation failed"); return -1; }
      const U64 seq = ++g.seq;
      if (mgLaunchIterScan (p, (const U32 *) (g.dIn + 16), total, (const U64 *) g.dIn, g.dSegK, g.dSegP, g.dOut, g.outEntries, g.dFlag, seq, g.st)) return -1;
      U64 *flag = g.hFlag;
      bool done = false;
      /* acquire loads: the block the kernel wrote before its release store of the flag is read after the flag is seen */
      for (int spin = 0 ; spin < (1 << 22) ; ++spin) { if (__atomic_load_n (flag, __ATOMIC_ACQUIRE) == seq) { done = true; break; } _mm_pause (); }
      if (!done)                                           /* a kernel that takes this long, or one that failed: ask the runtime */
        { hipError_t e = hipStreamSynchronize (g.st);
          if (e != hipSuccess) { mgHipFail (e, "iterator scan"); g.release (); return -1; }      /* (nothing of this scratch is reused after a failure) */
          if (__atomic_load_n (flag, __ATOMIC_ACQUIRE) != seq) { mgSetError ("iterator scan: no completion flag"); g.release (); return -1; }
        }
      const U64 n = g.hOut[0];
      if (n > g.outEntries) { want = n; continue; }
      const size_t bytes = (size_t) (n + 1) * 8 + (size_t) n * 4;
      U64 *blk = (U64 *) malloc (bytes + 8);
      if (!blk) return -1;
      memcpy (blk, g.hOut, bytes);
      *blkOut = blk;
      return 0;
    }
  mgSetError ("iterator scan: output capacity could not be established");
  return -1;
}

extern "C" int mgIterRequireDevice (void) { return mgEnsureDevice () ? -1 : 0; }

extern "C" void mgIterReleaseBuffers (void) { if (gIt.dev >= 0) gIt.release (); }
