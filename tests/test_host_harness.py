"""The host code's stand-alone sanitizer harnesses (tools/tsan_qpipe.sh, tools/tsan_textout.sh, tools/asan_seqio.sh): each compiles one
or two of the library's C files with a main of its own under ThreadSanitizer and / or AddressSanitizer + UBSan, with the device stubbed
by host memory, and checks what comes out.  Run here so that they keep linking: a script passes when it exits 0 and prints its own
success line.  No GPU, nothing loaded into Python; everything is written under tmp_path."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = """#include <pthread.h>
static void *f (void *v) { return v; }
int main (void) { pthread_t t; return pthread_create (&t, 0, f, 0) || pthread_join (t, 0); }
"""


def _need_sanitizers(tmp_path, *sets):
    """skip unless a thread can be started and joined under each -fsanitize= set on this machine (a program that has nothing to do with the code under test)"""
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    for san in sets:
        exe = str(tmp_path / "probe")
        try:
            ok = subprocess.run(["gcc", "-fsanitize=" + san, "-o", exe, str(src), "-lpthread"], capture_output=True).returncode == 0 \
                and subprocess.run([exe], capture_output=True, timeout=60).returncode == 0
        except (OSError, subprocess.TimeoutExpired):
            ok = False
        if not ok:
            pytest.skip("no working -fsanitize=%s on this machine" % san)


def _run(tmp_path, script, *args):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", script)] + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_tsan_qpipe(tmp_path):
    """mgQueryFile's pipe (mg_queryout.c): 60 batches on either side of the 20 000-read team threshold, empty reads among them, more pushed than the queues hold"""
    _need_sanitizers(tmp_path, "thread", "address,undefined")
    out = _run(tmp_path, "tsan_qpipe.sh")
    assert "-fsanitize=thread: output identical" in out and "-fsanitize=address,undefined: output identical" in out, out


def test_tsan_textout(tmp_path):
    """the reports' writer (mg_textout.c): calls that cross a piece, more pieces than blocks, a small piece in a large block"""
    _need_sanitizers(tmp_path, "thread", "address,undefined")
    out = _run(tmp_path, "tsan_textout.sh")
    assert "-fsanitize=thread: output identical (125829125 bytes)" in out and "-fsanitize=address,undefined: output identical (125829125 bytes)" in out, out


def test_asan_seqio(tmp_path):
    """the host parser (mg_seqio.c): three batch sizes by two thread counts give one digest"""
    _need_sanitizers(tmp_path, "address,undefined")
    out = _run(tmp_path, "asan_seqio.sh", "12000")
    assert "all six digests equal" in out, out
    digests = [l.split()[0] for l in out.splitlines() if l.endswith("  -")]
    assert len(digests) == 6 and len(set(digests)) == 1, out
