"""bench.py's command line, checked without a device: the extras of --full are opt-in, and asking for one of them without it
is refused before anything touches a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(*args):
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=300)


def test_full_is_an_option():
    r = _run("--help")
    assert r.returncode == 0 and "--full" in r.stdout


def test_dump_profile_needs_full():
    for args in (("--dump-profile", "p.json"), ("--full", "--no-roofline", "--dump-profile", "p.json")):
        r = _run(*args)
        assert r.returncode == 2 and "--dump-profile needs" in r.stderr, (args, r.returncode, r.stderr[-500:])
