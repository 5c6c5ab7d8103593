#!/bin/bash
# dev: the text parser (mg_seqio.c) under AddressSanitizer + UBSan on the CPU, over the golden text files
# and generated files: short-read FASTQ (plain and blocked gzip), records of exact multiples of the conversion unit.
# Compiled: mg_seqio.c + mg_knobs.c and a main that calls the parser -- the file loops of its callers live in mg_seqfiles.c, so
# nothing is stubbed.  Three batch sizes by two thread counts: the six digests must be equal.  Writes under $TMPDIR.
# usage: bash tools/asan_seqio.sh [reads of the generated FASTQ file: 120000; tests/test_host_harness.py asks for 12000, which still makes
#        batches on either side of the 4096 records at which the bookkeeping goes to the team]
set -e
R=$(cd "$(dirname "$0")/.." && pwd); B=${TMPDIR:-/tmp}/modgpu_asan_seqio; mkdir -p $B
READS=${1:-120000}
cat > $B/main.c <<'EOC'
#include <stdio.h>
#include <stdlib.h>
#include "modgpu.h"
int main (int argc, char **argv)
{
  for (int a = 2 ; a < argc ; ++a)
    { MgSeqReader *r = mgSeqOpen (argv[a]); if (!r) continue;
      MgSeqBatch b; unsigned long long sum = 0, ids = 0, n = 0;
      while (mgSeqNextBatch (r, atoll (argv[1]), &b))
        { for (int i = 0 ; i < b.nSeq ; ++i) { for (const char *p = b.names[i] ; *p ; ++p) ids = ids * 31 + (unsigned char) *p; ids = ids * 31 + (unsigned long long) (b.offsets[i + 1] - b.offsets[i]); }
          for (int64_t i = 0 ; i < b.total ; ++i) sum = sum * 131 + (unsigned char) b.bases[i];
          n += b.nSeq; mgSeqBatchFree (&b);
        }
      mgSeqClose (r);
      printf ("%s: %llu records, checksums %llx %llx\n", argv[a], n, ids, sum);
    }
  return 0;
}
EOC
gcc -g -O1 -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -I$R/include -I$R/modimizer_amd/csrc \
    $B/main.c $R/modimizer_amd/csrc/mg_seqio.c $R/modimizer_amd/csrc/mg_knobs.c -o $B/seqio_asan -lz -lpthread
python3 - $B $READS <<'EOP'
import sys
import numpy as np
B = sys.argv[1]
rng = np.random.default_rng(2)
with open(B + "/short.fq", "wb") as f:
    for i in range(int(sys.argv[2])):
        l = int(rng.integers(0, 200)); s = np.frombuffer(b"ACGTNacgtRY", np.uint8)[rng.integers(0, 11, l)].tobytes()
        f.write(b"@r%d x\n" % i + s + b"\n+\n" + b"I" * l + b"\n")
    f.write(b"@cut\nACG")
import struct, zlib
raw = open(B + "/short.fq", "rb").read()
with open(B + "/short.fq.bgz", "wb") as f:                 # the same text as blocked gzip
    for i in range(0, len(raw), 60000):
        ch = raw[i:i + 60000]; c = zlib.compressobj(1, zlib.DEFLATED, -15); pay = c.compress(ch) + c.flush()
        f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(pay) + 25) + pay + struct.pack("<II", zlib.crc32(ch), len(ch)))
    f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
# records whose raw sequence text is an exact multiple of the 1 MiB conversion unit (FASTA: newlines included)
L = np.frombuffer(b"ACGT", np.uint8)
with open(B + "/mult.fa", "wb") as f:
    for i, lines in enumerate((16384, 3, 32768, 16383)):
        s = L[rng.integers(0, 4, lines * 63)]
        f.write(b">m%d\n" % i + b"".join(s[j:j + 63].tobytes() + b"\n" for j in range(0, len(s), 63)))
with open(B + "/mult.fq", "wb") as f:
    for i, n in enumerate((1 << 20, 7, 2 << 20, (1 << 20) + 1)):
        f.write(b"@m%d\n" % i + L[rng.integers(0, 4, n)].tobytes() + b"\n+\n" + b"I" * n + b"\n")
EOP
G=$R/tests/golden
: > $B/digests.txt
for mb in 3000 777777 1000000000; do
  for t in 1 7; do
    MODGPU_PARSE_THREADS=$t $B/seqio_asan $mb $G/mixed.fa $G/mixed.fa.gz $G/mixed.fq $G/unterminated.fa $G/many.fa $B/short.fq $B/short.fq.bgz $B/mult.fa $B/mult.fq > $B/run.txt 2>&1
    grep -q "short.fq.bgz: $READS records" $B/run.txt            # (a run that parsed nothing would agree with itself, too)
    md5sum < $B/run.txt | tee -a $B/digests.txt
  done
done
if [ "$(sort -u $B/digests.txt | wc -l)" = 1 ] && [ "$(wc -l < $B/digests.txt)" = 6 ]; then echo "all six digests equal"
else echo "DIGESTS DIFFER"; exit 1; fi
