"""Host-only check of the fifth item of a handle's cache contract, the image-prompt K / V (csrc/cache_record.h; include/sdeo.h, "State a
handle keeps between calls"): tests/ip_cache_record_check.cpp is built against the header with the host g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program of its own, exactly as tests/test_cache_record_cpu.py builds and runs its program
(nothing is loaded into this process).  sdeo_set_ip_tokens makes every reader accepted, sdeo_configure makes them refused with the
library's whole message, sdeo_lora_commit leaves the item as it was, a refused check leaves the record equal to its copy, and the new
transitions leave the four other items alone.  tests/test_ip_adapter_gpu.py pins the same from the entry points, on the device."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_ip_cache_record(tmp_path):
    gxx = "/usr/bin/g++" if os.path.exists("/usr/bin/g++") else shutil.which("g++")
    assert gxx, "no host g++"
    exe = str(tmp_path / "ip_cache_record_check")
    # the sanitizer runtimes are linked statically: the program runs in whatever environment the suite runs in
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(HERE, "ip_cache_record_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ip_cache_record_check: ok" in run.stdout
