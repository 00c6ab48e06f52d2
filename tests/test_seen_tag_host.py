"""katome_amd/csrc/seen_tag.h -- the delta tag of a first-seen build's tagged records (reads of varying length) -- checked on the host
by tests/hostshim/seen_tag_host.cpp, a program of its own: round trips at the limits, the exchange of the two orientations, the
sub-window rule against a literal loop over a read's windows, and the ordering claim (minima taken record by record through the
tags are the minima of the true numbers, and pack again) on 10 000 random read sets.  Runs without a GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostshim", "seen_tag_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


def _run(exe, env=None):
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    word, checks = out.stdout.split()
    assert word == "ok" and int(checks) > 100000


def test_delta_tag(tmp_path):
    exe = str(tmp_path / "seen_tag_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe])
    _run(exe)


def test_delta_tag_under_asan_and_ubsan(tmp_path):
    probe = tmp_path / "t.c"
    probe.write_text("int main(void){return 0;}\n")
    try:
        subprocess.check_call(["gcc"] + SAN + [str(probe), "-o", str(tmp_path / "t")], stderr=subprocess.DEVNULL)
        have = subprocess.call([str(tmp_path / "t")], env=ENV) == 0
    except (subprocess.CalledProcessError, OSError):
        have = False
    if not have:
        pytest.skip("gcc sanitizer runtime not available")
    exe = str(tmp_path / "seen_tag_host_san")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + [SRC, "-o", exe])
    _run(exe, ENV)
