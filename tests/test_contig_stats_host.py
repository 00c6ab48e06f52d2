"""katome_amd/csrc/contig_stats.h (Contigs::stats, stats/contigs.rs:31-89) through the host shim: the reference's three pins, the
empty assembly, the tipping points of 0 where the reference panics, and random length lists against a restatement.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "hostshim", "collapse_exact_host.cpp")
    hdrs = [os.path.join(ROOT, "katome_amd", "csrc", h) for h in ("shrink_exact.h", "collapse_exact.h", "contig_stats.h", "multi_route.h", "env.h")]
    so = os.path.join(HERE, "hostshim", "libcollapse_exact_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def stats(shim, lengths, genome_length):
    """-> (rc, (n50, l50, n90, ng50))"""
    a = np.array(lengths, np.uint64)
    out = np.zeros(4, np.uint64)
    rc = shim.hs_contig_stats(a.ctypes.data_as(C.c_void_p), C.c_uint64(len(lengths)), C.c_uint64(genome_length), out.ctypes.data_as(C.c_void_p))
    return rc, tuple(int(x) for x in out)


def restated(lengths, genome_length):
    """stats/contigs.rs:31-89; None where `.last().unwrap()` panics"""
    if not lengths:
        return (0, 0, 0, 0)
    c = sorted(lengths)
    total = sum(c)

    def n_metrics(tip):
        acc, last = 0, None
        for x in c:
            if acc >= tip:
                break
            last, acc = x, acc + x
        return last
    n50, n90, ng50 = n_metrics(total // 2), n_metrics(int(0.1 * float(total))), n_metrics(genome_length // 2)
    if None in (n50, n90, ng50):
        return None
    acc, l50 = 0, 0
    for i, x in enumerate(reversed(c)):
        if acc >= total // 2:
            break
        l50, acc = i + 1, acc + x
    return (n50, l50, n90, ng50)


def test_reference_pins(shim):
    """stats/contigs.rs:100-147"""
    for lengths, want in (([2, 3, 4, 5, 6, 7, 8, 9, 10], (7, 3, 3, 7)), ([80, 70, 50, 40, 30, 20], (70, 2, 30, 70)),
                          ([80, 70, 50, 40, 30, 20, 10, 5], (50, 3, 20, 50))):
        assert stats(shim, lengths, sum(lengths)) == (0, want)
        assert restated(lengths, sum(lengths)) == want


def test_empty(shim):
    assert stats(shim, [], 0) == (0, (0, 0, 0, 0))
    assert stats(shim, [], 1000) == (0, (0, 0, 0, 0))


def test_zero_tipping_points(shim):
    """a tipping point of 0 with contigs present: the reference panics; here the code names which one (1 n50, 2 n90, 3 ng50)"""
    assert stats(shim, [50, 60], 0)[0] == 3
    assert stats(shim, [50, 60], 1)[0] == 3
    assert stats(shim, [50, 60], 2)[0] == 0
    assert stats(shim, [1], 100)[0] == 1            # sum / 2 == 0
    assert stats(shim, [4, 5], 100)[0] == 2         # 0.1 * 9 truncates to 0
    assert restated([4, 5], 100) is None and restated([50, 60], 1) is None


def test_random_lists(shim):
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(1, 60))
        lengths = [int(x) for x in rng.integers(1, int(rng.choice([5, 200, 100000])), n)]
        genome = int(rng.integers(2, 3 * sum(lengths) + 3))
        want = restated(lengths, genome)
        rc, got = stats(shim, lengths, genome)
        assert (rc == 0) == (want is not None)
        if want is not None:
            assert got == want


def test_library_symbol_names_the_tipping_point():
    """katome_contig_stats_of (the library's host symbol; no device is touched): the pins, zeros for no contigs, and
    KATOME_E_ARG with a message that names the tipping point where the reference panics"""
    from katome_amd.build import KatomePanic, contig_stats
    assert contig_stats([2, 3, 4, 5, 6, 7, 8, 9, 10], 54) == (7, 3, 3, 7)
    assert contig_stats([], 0) == (0, 0, 0, 0)
    for lengths, genome, which in (([50, 60], 0, "ng50"), ([50, 60], 1, "ng50"), ([1], 100, "n50"), ([4, 5], 100, "n90")):
        with pytest.raises(KatomePanic) as e:
            contig_stats(lengths, genome)
        assert e.value.status == -7 and e.value.name == "E_ARG" and which in e.value.message
    assert contig_stats([50, 60], 2) == restated([50, 60], 2)
