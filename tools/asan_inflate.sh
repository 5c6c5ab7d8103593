#!/bin/bash
# dev: the raw-deflate decoder (csrc/mg_inflate_core.h) alone under AddressSanitizer + UBSan on the CPU, between guard pages, over the
# whole corpus of tests/test_inflate_host.py, the corrupt members included (tools/inflate_host_check.c).  usage: bash tools/asan_inflate.sh
set -e
cd "$(dirname "$0")/.."
B=build/asan; mkdir -p $B
python3 -c "from tests import test_inflate_host as t; print(len(t.write_corpus('$B/inflate_corpus.bin')), 'members written')"
gcc -g -O1 -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -static-libasan -static-libubsan \
    -Imodimizer_amd/csrc tools/inflate_host_check.c -o $B/inflate_host_check
$B/inflate_host_check $B/inflate_corpus.bin | tail -1
