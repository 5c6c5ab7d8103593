#!/bin/bash
# dev: the bookkeeping of MgDevScratch and MgDevBuf (mg_common.h) under AddressSanitizer + UBSan, on the CPU: hipMalloc / hipFree are stubs
# that count and can fail the n-th allocation.  The shapes of the calls that use them are walked with every allocation failing in turn:
# an attempt's arrays freed before the next attempt allocates (mgReadsetSeedsDevice), arrays handed on with take (), a scratch that is a
# member (the set text parser), a buffer that grows, fails and is dropped.  Each walk ends with frees = allocations - what was handed on.
set -e
R=$(cd "$(dirname "$0")/.." && pwd); D=${TMPDIR:-/tmp}/modgpu_asan_scratch; mkdir -p $D
cat > $D/main.cpp <<'EOS'
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include "mg_common.h"
static std::set<void *> live; static long allocs, frees, failAt; static char err[256];
hipError_t hipMalloc (void **p, size_t n) { if (++allocs == failAt) { *p = 0; return hipErrorOutOfMemory; } *p = malloc (n ? n : 1); live.insert (*p); return hipSuccess; }
hipError_t hipFree (void *p) { if (!p) return hipSuccess; if (!live.erase (p)) { printf ("free of %p: not live\n", p); abort (); } ++frees; free (p); return hipSuccess; }
hipError_t hipGetLastError (void) { return hipSuccess; }
void mgSetError (const char *fmt, ...) { snprintf (err, sizeof (err), "%s", fmt); }
extern "C" const char *mgLastError (void) { return err; }
MgStatus mgHipFail (hipError_t e, const char *what) { snprintf (err, sizeof (err), "HIP error %d in %s", (int) e, what); return MG_ERR_HIP; }
#define CHECK(c) do { if (!(c)) { printf ("line %d: %s (allocation %ld failing)\n", __LINE__, #c, failAt); exit (1); } } while (0)

/* mgReadsetSeedsDevice: two attempts when retry, the winners adopted, nine more arrays, two of them handed on */
static int seeds (bool retry, U32 **hitOut, unsigned short **dxOut)
{
  MgDevScratch scratch ("seeds");
  U32 *ix, *pos, *rid, *a[6], *hit; unsigned short *dx; size_t guess = 100;
  for (int attempt = 0 ; ; ++attempt)
    { CHECK (live.empty ());                               /* the first guess is gone before the second is made */
      MgDevScratch s (scratch.what);
      if (s.get (&ix, guess) || s.get (&pos, guess) || s.get (&rid, guess)) return -1;
      if (!retry || attempt) { scratch.adopt (s.take (ix)); scratch.adopt (s.take (pos)); scratch.adopt (s.take (rid)); break; }
      guess = 1000;
    }
  CHECK (live.size () == 3);
  for (int i = 0 ; i < 6 ; ++i) if (scratch.get (&a[i], 7 + i)) return -1;
  if (scratch.get (&hit, 50) || scratch.get (&dx, 50)) return -1;
  *hitOut = scratch.take (hit); *dxOut = scratch.take (dx);
  return 0;
}
/* the set text parser: the scratch a member of the call's owner, three arrays out through take () */
struct Owner { MgDevScratch scratch { "parse" }; U64 *key = 0; U16 *depth = 0; U8 *info = 0; };
static int parse (U64 **key, U16 **depth, U8 **info)
{
  Owner b; char *text[2]; U32 *t[5];
  for (int i = 0 ; i < 2 ; ++i) if (b.scratch.get (&text[i], 4096)) return -1;
  for (int i = 0 ; i < 5 ; ++i) if (b.scratch.get (&t[i], 33)) return -1;
  if (b.scratch.get (&b.key, 10) || b.scratch.get (&b.depth, 10) || b.scratch.get (&b.info, 10)) return -1;
  *key = b.scratch.take (b.key); *depth = b.scratch.take (b.depth); *info = b.scratch.take (b.info);
  return 0;
}
/* merge (three arrays, then the core's two), prune, fill: gets in a row, everything freed on the way out */
static int nested (void)
{
  MgDevScratch outer ("second set"); U64 *v; U16 *d; U8 *i;
  if (outer.get (&v, 9) || outer.get (&d, 9) || outer.get (&i, 9)) return -1;
  MgDevScratch core ("merge"); U8 *i1; U32 *idx; char *work;
  if (core.get (&i1, 20) || core.get (&idx, 9) || core.get (&work, 0)) return -1;
  return 0;
}
int main (void)
{
  long walks = 0;
  for (int shape = 0 ; shape < 4 ; ++shape)
    for (failAt = 1 ; ; ++failAt, ++walks)
      { allocs = frees = 0; err[0] = 0;
        void *out[3] = { 0, 0, 0 };
        const int rc = shape < 2 ? seeds (shape == 1, (U32 **) &out[0], (unsigned short **) &out[1])
                     : shape == 2 ? parse ((U64 **) &out[0], (U16 **) &out[1], (U8 **) &out[2]) : nested ();
        long handed = 0; for (void *p : out) if (p) { ++handed; CHECK (live.count (p)); }
        const long made = allocs - (rc ? 1 : 0);           /* the failing one made nothing */
        CHECK (rc == (allocs >= failAt ? -1 : 0) && (rc ? !handed && err[0] : !err[0]));
        CHECK (frees == made - handed && (long) live.size () == handed);
        for (void *p : out) (void) hipFree (p);
        CHECK (live.empty ());
        if (!rc) break;
      }
  /* MgDevBuf: grows to the caller's number, not below; a failed growth leaves nothing; drop () */
  failAt = 0; allocs = frees = 0;
  MgDevBuf<U64> b;
  CHECK (!b.reserve (10, 12, "buf") && b.p && b.cap == 12 && allocs == 1);
  U64 *was = b.p;
  CHECK (!b.reserve (12, 99, "buf") && b.p == was && b.cap == 12 && allocs == 1);
  CHECK (!b.reserve (13, 13, "buf") && b.cap == 13 && allocs == 2 && frees == 1 && live.size () == 1);
  failAt = 3;
  CHECK (b.reserve (14, 28, "buf") == MG_ERR_HIP && !b.p && !b.cap && live.empty ());
  failAt = 0;
  CHECK (!b.reserve (1, 1, "buf") && b.cap == 1);
  b.drop (); b.drop ();
  CHECK (!b.p && !b.cap && live.empty () && frees == 3);
  printf ("asan_scratch ok: %ld walks\n", walks);
  return 0;
}
EOS
g++ -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$R/include -I$R/modimizer_amd/csrc \
    -Wall -Wno-unused-function -o $D/t $D/main.cpp
$D/t
