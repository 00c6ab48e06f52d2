"""The host results of katome_amd/csrc/host_build.cpp -- the owner every katome_*_free releases, the handle that holds a result
under construction, the copier that fills its arrays and keeps the first failure -- built for the host with
-fsanitize=address,undefined and run as a program of its own (tests/hostshim/host_results_selftest.cpp): results made in full
and freed through the public free, arrays of 0 bytes, a copy failing half-way with the handle freeing what was taken, NULL."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.mark.skipif(not os.path.isdir("/opt/rocm/include"), reason="HIP headers (for the shared declarations) not installed")
def test_owner_and_copier_under_asan(tmp_path):
    exe = str(tmp_path / "host_results_selftest")
    # (no skip for a missing sanitizer runtime: one that does not build or run is a failure to see)
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                                                          os.path.join(ROOT, "katome_amd", "csrc", "ingest.cpp"),
                                                          os.path.join(HERE, "hostshim", "host_results_selftest.cpp"), "-o", exe, "-lpthread"])
    out = subprocess.check_output([exe], env=ENV, timeout=300).split()
    assert out[0] == b"ok" and int(out[1]) > 3000
