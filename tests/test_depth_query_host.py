"""The query scanner of katome_depth_paths (ingest.cpp scan_query / ingest_query_files) from a stand-alone program with its own main,
built with -fsanitize=address,undefined on the CPU: literal cases in memory, then files -- every record kept, in file order."""
import os
import subprocess

import pytest

from test_sanitizers import ENV, HERE, ROOT, SAN, _have_sanitizers


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("depth_query"))
    if not os.path.isdir("/opt/rocm/include"):
        pytest.skip("HIP headers (for the shared declarations) not installed")
    if not _have_sanitizers(tmp):
        pytest.skip("gcc sanitizer runtime not available")
    exe = os.path.join(tmp, "depth_query_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "katome_amd", "csrc", "ingest.cpp"),
                                                         os.path.join(HERE, "hostshim", "depth_query_selftest.cpp"), "-o", exe, "-lpthread"])
    return exe


def test_literal_cases_run_clean(selftest):
    out = subprocess.check_output([selftest, "0"], env=ENV, timeout=300).split()
    assert out[0] == b"ok" and int(out[1]) == 16


def test_files_keep_every_record_in_order(selftest, tmp_path):
    fa, fq = tmp_path / "q.fa", tmp_path / "q.fq"
    fa.write_text(">multi\nACGTAC\nGGTT\nA\n>n\nACGTNNACGT\n>short\nAC\n>empty\n>tail\nTTTT\n")
    fq.write_text("@multi\nACGTACGGTTA\n+\nIIIIIIIIIII\n@n\nACGTNNACGT\n+\nIIIIIIIIII\n@short\nAC\n+\nII\n@empty\n\n+\n\n@tail\nTTTT\n+\nIIII\n")
    run = lambda ft, *files: subprocess.check_output([selftest, str(ft)] + [str(f) for f in files], env=ENV, timeout=300).decode().splitlines()[1]
    assert run(0, fa) == "0 5 27: 11 10 2 0 4"
    assert run(1, fq) == "0 5 27: 11 10 2 0 4"
    assert run(0, fa, fa) == "0 10 54: 11 10 2 0 4 11 10 2 0 4"
    assert run(2, fa).split()[0] == "-7"                                    # BFCounter is no query type
    assert run(0, tmp_path / "missing.fa").split()[0] == "-1"              # the ingest's own status: the path does not resolve
    assert run(0, tmp_path).split()[0] == "-2"                              # a directory
    assert run(0, fq).split()[0] == "-5"                                    # a FASTQ read as FASTA: not a record start
