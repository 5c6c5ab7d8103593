/* oracle/devsort_probe.hip — TEST INFRASTRUCTURE ONLY.
 *
 * libdevsortprobe.so: the two device-wide primitives of modimizer_amd/csrc/mg_devsort.h (mgExclusiveScan, mgRefStableSort) and the
 * host arithmetic next to them (mgKeyBits, mgScanScratchWords) behind plain entry points, so that tests/test_gpu_devsort.py can hold
 * them against numpy on inputs of its own choosing: every number of sort passes, ragged last rounds, waves of one digit, equal keys
 * across the 2048- and 8192-element lines, sums of exactly 2^32 - 1, n around the multiples of 4096.  The library's callers reach
 * them only with what a read set or a reference happens to hold.
 *
 * Host code only, no kernel: the probe is LINKED against modimizer_amd/libmodgpu.so, so what runs is the library's own binary, not a
 * second compile of mg_devsort.hip (MgDevScratch is inline in mg_common.h; its mgHipFail comes from the library too).
 *
 * Every entry point takes HOST pointers and works on the null stream: it allocates, copies in, calls, copies back, frees, and
 * returns 0 or the MgStatus (-1: refused).  The Makefile bakes a hash of this file, mg_devsort.h and mg_common.h into it
 * (devsort_probe.inc); devsortProbeHash () returns it and the tests compare it with the tree's. */
#include "../modimizer_amd/csrc/mg_devsort.h"
#include "devsort_probe.inc"

static const char gProbeMarker[] = "DEVSORT_PROBE_HASH=" DEVSORT_PROBE_HASH;
extern "C" const char *devsortProbeHash (void) { return gProbeMarker + 19; }

extern "C" int devsortProbeKeyBits (U64 maxKey) { return mgKeyBits (maxKey); }
extern "C" U64 devsortProbeScratchWords (U64 n) { return (U64) mgScanScratchWords (n); }

#define PROBE_HIP(call) do { if ((call) != hipSuccess) return (int) scratch.fail (); } while (0)

/* out: guard + n + guard words of the caller's; the whole of it goes up before the call and comes back after it, mgExclusiveScan's
 * out[] being the n in the middle.  inPlace: in[] IS out[], so the middle of out holds the input and in is not read.  Otherwise in
 * (n words) goes up and comes back into the caller's array after the call: the test checks that it is what it was.  wantTotal: the
 * scan is given a host word for the total and *total is that; otherwise it is given none and *total is left alone. */
extern "C" int devsortProbeScan (const U32 *in, U32 *out, U64 n, U64 guard, int inPlace, int wantTotal, U32 *total)
{
  if (n >= ((U64) 1 << 31) || guard >= ((U64) 1 << 20)) return -1;
  MgDevScratch scratch ("devsort probe: scan");
  const size_t outWords = (size_t) (n + 2 * guard);
  U32 *dIn, *dOut;
  if (scratch.get (&dIn, (size_t) n + 4) || scratch.get (&dOut, outWords + 4)) return (int) MG_ERR_HIP;
  if (!inPlace && n) PROBE_HIP (hipMemcpy (dIn, in, (size_t) n * 4, hipMemcpyHostToDevice));
  if (outWords) PROBE_HIP (hipMemcpy (dOut, out, outWords * 4, hipMemcpyHostToDevice));
  U32 sum = 0;
  const MgStatus s = mgExclusiveScan (scratch, inPlace ? dOut + guard : dIn, dOut + guard, n, 0, wantTotal ? &sum : (U32 *) 0);
  if (s) return (int) s;
  PROBE_HIP (hipStreamSynchronize (0));
  if (!inPlace && n) PROBE_HIP (hipMemcpy ((U32 *) in, dIn, (size_t) n * 4, hipMemcpyDeviceToHost));
  if (outWords) PROBE_HIP (hipMemcpy (out, dOut, outWords * 4, hipMemcpyDeviceToHost));
  if (wantTotal) *total = sum;
  return 0;
}

/* keys[n], vals[n] or 0: up; mgRefStableSort; out[n]: what it made.  keysBack[n] and (vals != 0) valsBack[n]: the device's input arrays
 * after the sort, which must not have touched them.  n == 0 is refused: every caller guards it, and a launch of no workgroups is not
 * something to try. */
extern "C" int devsortProbeSort (const U32 *keys, const U32 *vals, U32 n, int keyBits, U32 *out, U32 *keysBack, U32 *valsBack)
{
  if (!n || n >= ((U32) 1 << 31) || keyBits < 1 || keyBits > 32) return -1;
  MgDevScratch scratch ("devsort probe: sort");
  U32 *dKeys, *dVals = 0, *dOut = 0;
  if (scratch.get (&dKeys, n) || (vals && scratch.get (&dVals, n))) return (int) MG_ERR_HIP;
  PROBE_HIP (hipMemcpy (dKeys, keys, (size_t) n * 4, hipMemcpyHostToDevice));
  if (vals) PROBE_HIP (hipMemcpy (dVals, vals, (size_t) n * 4, hipMemcpyHostToDevice));
  const MgStatus s = mgRefStableSort (scratch, dKeys, dVals, n, keyBits, &dOut, 0);
  if (s) return (int) s;
  PROBE_HIP (hipMemcpy (out, dOut, (size_t) n * 4, hipMemcpyDeviceToHost));
  PROBE_HIP (hipMemcpy (keysBack, dKeys, (size_t) n * 4, hipMemcpyDeviceToHost));
  if (vals) PROBE_HIP (hipMemcpy (valsBack, dVals, (size_t) n * 4, hipMemcpyDeviceToHost));
  return 0;
}
