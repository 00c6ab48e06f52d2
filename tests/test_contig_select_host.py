"""katome_amd/csrc/contig_select.h -- Contigs::stats as four radix selections over sums of all contigs -- against contig_stats.h's
sorted scans, through the host shim: a Python loop plays the four passes the way csrc/dist_text.hip does, with the list cut into
shards whose bins are added up.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GIANT = 2 ** 32 - 1


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "hostshim", "contig_select_host.cpp")
    hdrs = [os.path.join(ROOT, "katome_amd", "csrc", h) for h in ("contig_select.h", "contig_stats.h")]
    so = os.path.join(HERE, "hostshim", "libcontig_select_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.hs_select_new.restype = C.c_void_p
    lib.hs_select_new.argtypes = [C.c_uint32, C.c_uint64]
    lib.hs_select_free.argtypes = [C.c_void_p]
    lib.hs_select_pass.argtypes = [C.c_void_p, C.c_void_p]
    lib.hs_select_step.argtypes = [C.c_void_p, C.c_void_p]
    lib.hs_select_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.hs_select_reference.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    return lib


def selected(shim, shards, k, genome):
    """the passes over the shards' k-mer counts (uint32 arrays) -> (rc, (n50, l50, n90, ng50)), and how many passes ran"""
    h = shim.hs_select_new(k, genome)
    prefix = np.zeros(4, np.uint32)
    passes = 0
    try:
        while True:
            p = shim.hs_select_pass(h, prefix.ctypes.data)
            shift = 24 - 8 * p
            bins = np.zeros((4, 256, 2), np.uint64)
            for m in shards:                                  # one "rank": its own contigs only
                for s in range(4):
                    sel = m if p == 0 else m[(m.astype(np.uint64) >> np.uint64(shift + 8)) == np.uint64(prefix[s])]
                    d = ((sel >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
                    np.add.at(bins[s, :, 0], d, np.uint64(1))
                    np.add.at(bins[s, :, 1], d, sel.astype(np.uint64))
            passes += 1
            if not shim.hs_select_step(h, bins.ctypes.data):
                break
        out = np.zeros(4, np.uint64)
        rc = shim.hs_select_result(h, out.ctypes.data)
        return (rc, tuple(int(x) for x in out)), passes
    finally:
        shim.hs_select_free(h)


def reference(shim, kmers, k, genome):
    lengths = np.asarray(kmers, np.uint64) + np.uint64(k - 1)
    out = np.zeros(4, np.uint64)
    rc = shim.hs_select_reference(lengths.ctypes.data, len(lengths), genome, out.ctypes.data)
    return rc, tuple(int(x) for x in out)


def cut(rng, kmers, n_shards, some_empty):
    """the list dealt to n_shards shards in random order; with some_empty a few shards get nothing"""
    m = np.asarray(kmers, np.uint32)
    owners = np.arange(n_shards)
    if some_empty and n_shards > 1:
        owners = rng.choice(n_shards, size=max(1, n_shards // 2), replace=False)
    who = rng.choice(owners, size=len(m))
    return [m[who == r] for r in range(n_shards)]


def check(shim, rng, kmers, k, genome, n_shards=None, some_empty=False):
    n_shards = int(rng.integers(1, 9)) if n_shards is None else n_shards
    want = reference(shim, kmers, k, genome)
    got, passes = selected(shim, cut(rng, kmers, n_shards, some_empty), k, genome)
    assert got == want, (list(map(int, kmers))[:40], k, genome, n_shards)
    assert passes == (4 if want[0] != 1 and len(kmers) else 1)
    return want


def genomes(kmers, k):
    total = int(sum(int(x) + k - 1 for x in kmers))
    return (0, 1, 2, total, 3 * total)


def test_named_cases(shim):
    rng = np.random.default_rng(5)
    cases = {
        "all equal": ([7] * 9, 31), "all equal, two": ([3, 3], 5), "n = 1": ([12], 21), "n = 1, giant": ([GIANT], 31),
        "crossing inside a tie group": ([5, 5, 5, 5, 1, 1], 5), "ties at the top": ([9, 9, 9, 2, 2, 2, 2, 2, 2], 4),
        "one giant": ([GIANT] + [3] * 50, 31), "two giants": ([GIANT, GIANT, 1, 2, 3], 63), "giant and ties": ([GIANT, 2 ** 24, 2 ** 24, 2 ** 16, 255, 256], 31),
        "reference pin 1": ([2, 3, 4, 5, 6, 7, 8, 9, 10], 1), "reference pin 2": ([80, 70, 50, 40, 30, 20], 1),
        "reference pin 3": ([80, 70, 50, 40, 30, 20, 10, 5], 1),
    }
    for name, (kmers, k) in cases.items():
        for genome in genomes(kmers, k):
            for n_shards in (1, 2, 5, 8):
                check(shim, rng, kmers, k, genome, n_shards, some_empty=n_shards == 8)
    # stats/contigs.rs:100-147, lengths given directly (k = 1: a contig's length is its k-mer count)
    assert selected(shim, [np.array([2, 3, 4, 5, 6, 7, 8, 9, 10], np.uint32)], 1, 54)[0] == (0, (7, 3, 3, 7))
    assert selected(shim, [np.array([80, 70, 50], np.uint32), np.array([40, 30, 20], np.uint32)], 1, 290)[0] == (0, (70, 2, 30, 70))


def test_error_codes(shim):
    """a tipping point of 0: contig_stats()'s 1 (n50), 2 (n90), 3 (ng50), in its order, with the fields it had filled in by then"""
    rng = np.random.default_rng(6)
    assert check(shim, rng, [1], 1, 100)[0] == 1                 # sum / 2 == 0
    assert check(shim, rng, [1], 1, 0)[0] == 1                   # ... found before ng50's
    assert check(shim, rng, [3, 4], 2, 100)[0] == 2              # 0.1 * 9 truncates to 0
    assert check(shim, rng, [3, 4], 2, 0)[0] == 2
    assert check(shim, rng, [50, 60], 5, 0)[0] == 3
    assert check(shim, rng, [50, 60], 5, 1)[0] == 3
    assert check(shim, rng, [50, 60], 5, 2)[0] == 0
    assert check(shim, rng, [], 31, 0) == (0, (0, 0, 0, 0))      # no contigs: zeros, whatever the genome
    assert check(shim, rng, [], 31, 1000, n_shards=8) == (0, (0, 0, 0, 0))


def test_random_lists(shim):
    rng = np.random.default_rng(7)
    codes = set()
    lists = 0
    for i in range(3200):
        n = int(rng.choice([1, 2, 3, int(rng.integers(1, 40)), int(rng.integers(40, 200))]))
        top = int(rng.choice([2, 4, 300, 70000, 2 ** 24 + 5, 2 ** 32]))      # few values: ties; many: every digit in play
        kmers = rng.integers(1, top, n, dtype=np.uint64).astype(np.uint32)
        if i % 7 == 0:
            kmers[int(rng.integers(0, n))] = GIANT
        if i % 11 == 0:
            kmers[:] = kmers[0]
        k = int(rng.choice([1, 2, 5, 31, 63]))
        gs = genomes(kmers, k)
        genome = int(gs[i % 5]) if i % 3 else int(rng.integers(0, 3 * gs[3] + 3))
        codes.add(check(shim, rng, kmers, k, genome, some_empty=i % 4 == 0)[0])
        lists += 1
    assert lists >= 3000 and codes == {0, 1, 2, 3}
