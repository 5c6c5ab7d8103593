#!/bin/bash
# dev: the raw-deflate encoder (csrc/mg_deflate_core.h) alone under AddressSanitizer + UBSan on the CPU, between guard pages, over the
# whole corpus of tests/test_deflate_host.py (tools/deflate_host_check.c: a stand-alone program).  usage: bash tools/asan_deflate.sh
set -e
cd "$(dirname "$0")/.."
B=build/asan; mkdir -p $B
python3 -c "from tests import test_deflate_host as t; print(len(t.write_corpus('$B/deflate_corpus.bin')), 'blocks written')"
gcc -g -O1 -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -static-libasan -static-libubsan \
    -Imodimizer_amd/csrc tools/deflate_host_check.c -o $B/deflate_host_check
$B/deflate_host_check $B/deflate_corpus.bin | tail -1
