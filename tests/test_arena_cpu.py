"""Host-only checks of the activation arena and the architecture plans of the network executor (csrc/arena.h, csrc/net_plan.h):
tests/arena_check.cpp is built against the two headers with the host g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run
as a program of its own, in the environment of the suite (nothing is loaded into this process).  It checks that live arena blocks never overlap and stay 256-byte
aligned over a fixed sequence of 10,000 alloc / release calls, that the plan is reproducible and survives the copy-and-rewind
build_shared_prefix and the decoder forms rely on, that a view is never owned, and that make_uplan agrees with spec.unet_plan, whose
input_block_chans / input_block_ds it receives on the command line."""
import os
import shutil
import subprocess

from stablediffusioneo_amd import spec

HERE = os.path.dirname(os.path.abspath(__file__))


def test_arena_and_plans(tmp_path):
    gxx = "/usr/bin/g++" if os.path.exists("/usr/bin/g++") else shutil.which("g++")
    assert gxx, "no host g++"
    exe = str(tmp_path / "arena_check")
    # the sanitizer runtimes are linked statically: the program runs in whatever environment the suite runs in
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(HERE, "arena_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    plan = spec.unet_plan(spec.UNET_SD15)
    assert len(plan.input_block_chans) == 12
    run = subprocess.run([exe, ",".join(map(str, plan.input_block_chans)), ",".join(map(str, plan.input_block_ds))],
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "arena_check: ok" in run.stdout
