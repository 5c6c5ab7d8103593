#!/usr/bin/env python3
"""Generate tests/golden/text_* by running the REFERENCE ITSELF (oracle/_ref/modutils_ref, built from the reference tree by
oracle/Makefile): modutils -rt / -wt (modutils.c:169-199).
Re-run with:  python tests/golden/make_golden_text.py

Per tag of util.MODUTILS_TAGS (B k w s), with dump = the -wt file of  -c B k w s -a reads.fa -a reads2.fa  (modutils_<tag>.dump*):
  text_<tag>.rt.mod          modutils_ref -rt dump -w text_<tag>.rt.mod   (gzip, as its fzopen writes it)
  text_<tag>.rt.stdout.txt   what that run prints, without the timing lines (make_golden.strip_timing's rule)
The hand-written tables text_dups.txt, text_loose.txt, text_long.txt (committed inputs, described in tests/test_gpu_settext.py):
  text_<name>.dump.txt       modutils_ref -rt text_<name>.txt -wt text_<name>.dump.txt
text_errors.json: for every case of ERRORS below the input (null: no such file) and what the reference prints after "FATAL ERROR: ",
without the newline die() adds (utils.c:19-30); the file's own name appears as <FILE>.  The case `long_token` overruns a static
buffer in the reference (undefined behaviour): its message is the library's own and is not run here.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import util  # noqa: E402

MU = os.path.join(ROOT, "oracle", "_ref", "modutils_ref")
KMER = "acgtacgtacgtacgtacgta"
HDR = "modset bits %s size %s k %s w %s seed 17\n"
LINE = "%d\t%s\t%s\t%d\n"
ERRORS = [
    ("depth_not_a_number", HDR % (20, 4, 21, 64) + LINE % (1, KMER, "5", 1) + LINE % (2, KMER[::-1], "x", 1) + LINE % (3, "g" * 21, "2", 0), None),
    ("fewer_lines", HDR % (20, 5, 21, 64) + LINE % (1, KMER, "5", 1), None),
    ("bits_19", HDR % (19, 2, 21, 64) + LINE % (1, KMER, "5", 1), None),
    ("size_too_big", HDR % (20, 300000, 21, 64) + LINE % (1, KMER, "5", 1), None),
    ("size_negative", HDR % (20, -5, 21, 64) + LINE % (1, KMER, "5", 1), None),
    ("k_32", HDR % (20, 2, 32, 64) + LINE % (1, KMER, "5", 1), None),
    ("w_0", HDR % (20, 2, 21, 0) + LINE % (1, KMER, "5", 1), None),
    ("missing_file", None, None),
    ("mangled_header", "modset bitz 20 size 2 k 21 w 64 seed 17\n" + LINE % (1, KMER, "5", 1), None),
    ("long_token", HDR % (20, 3, 21, 64) + LINE % (1, "acgt" * 10, "5", 1) + LINE % (2, KMER, "5", 1), "bad line 2"),
]


def strip_timing(text):
    return "\n".join(l for l in text.splitlines() if not l.startswith("user\t") and "resources used" not in l
                     and not l.startswith("total resources")) + "\n"


def run(cmd, cwd, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    assert (r.returncode == 0) == ok, (cmd, r.returncode, r.stderr[-2000:])
    return r


def main():
    assert os.path.exists(MU), "needs oracle/_ref/modutils_ref (only buildable where the reference tree exists)"
    tmp = tempfile.mkdtemp()
    try:
        for name in ("reads.fa", "reads2.fa"):
            shutil.copy(os.path.join(HERE, name), tmp)
        for tag, (B, k, w, s) in util.MODUTILS_TAGS.items():
            run([MU, "-o", "log.txt", "-c", str(B), str(k), str(w), str(s), "-a", "reads.fa", "-a", "reads2.fa", "-wt", "dump.txt"], tmp)
            util.check_dump(open(os.path.join(tmp, "dump.txt")).read(), "modutils_%s.dump.txt" % tag)      # the committed golden's text
            mod = "text_%s.rt.mod" % tag
            r = run([MU, "-rt", "dump.txt", "-w", mod], tmp)
            shutil.copy(os.path.join(tmp, mod), os.path.join(HERE, mod))
            open(os.path.join(HERE, "text_%s.rt.stdout.txt" % tag), "w").write(strip_timing(r.stdout))
            print(mod, os.path.getsize(os.path.join(HERE, mod)), "bytes")
            # -rt then -wt gives the dump back
            run([MU, "-o", "log.txt", "-rt", "dump.txt", "-wt", "again.txt"], tmp)
            assert open(os.path.join(tmp, "again.txt")).read() == open(os.path.join(tmp, "dump.txt")).read()
        for name in ("dups", "loose", "long"):
            shutil.copy(os.path.join(HERE, "text_%s.txt" % name), tmp)
            run([MU, "-o", "log.txt", "-rt", "text_%s.txt" % name, "-wt", "text_%s.dump.txt" % name], tmp)
            shutil.copy(os.path.join(tmp, "text_%s.dump.txt" % name), HERE)
            print("text_%s.dump.txt" % name, open(os.path.join(HERE, "text_%s.dump.txt" % name)).readline().strip())
        cases = []
        for name, text, own in ERRORS:
            fn = "err_%s.txt" % name
            if text is not None:
                open(os.path.join(tmp, fn), "w").write(text)
            if own is None:
                err = run([MU, "-o", "log.txt", "-rt", fn], tmp, ok=False).stderr
                assert "FATAL ERROR: " in err and err.endswith("\n"), err
                msg, ref = err[err.index("FATAL ERROR: ") + len("FATAL ERROR: "):-1].replace(fn, "<FILE>"), True
            else:
                msg, ref = own, False
            cases.append({"name": name, "input": text, "message": msg, "from_reference": ref})
            print(name, repr(msg))
        json.dump(cases, open(os.path.join(HERE, "text_errors.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
