"""Host-only check of the cache contract of a handle (csrc/cache_record.h; include/sdeo.h, "State a handle keeps between calls"):
tests/cache_record_check.cpp is built against the header with the host g++ under AddressSanitizer + UndefinedBehaviorSanitizer and
run as a program of its own, in the environment of the suite (nothing is loaded into this process).  It walks the table of
include/sdeo.h row by row (after each "filled by" transition every reader is accepted, after each "cleared by" one refused with the
library's whole message, after any other transition accepted as before), the epoch rule of the context K / V, the staged latent, stale
against unset, that a refused check leaves the record equal to its copy, and 20,000 random transitions and checks against a model of
what each cache holds.  tests/test_cache_contract_gpu.py pins the same contract from the entry points, on the device."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cache_record(tmp_path):
    gxx = "/usr/bin/g++" if os.path.exists("/usr/bin/g++") else shutil.which("g++")
    assert gxx, "no host g++"
    exe = str(tmp_path / "cache_record_check")
    # the sanitizer runtimes are linked statically: the program runs in whatever environment the suite runs in
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(HERE, "cache_record_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "cache_record_check: ok" in run.stdout
