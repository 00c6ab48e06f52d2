"""What the sharded GFA (katome_amd/csrc/dist_gfa.hip) rests on that needs no GPU: the directory arithmetic of dist_gfa_dir.h
against plain Python, and the numbered model of tests/dist_gfa_model.py against gfa_model.gfa_text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dist_gfa_model as dm
import gfa_model

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "hostshim", "dist_gfa_dir_host.cpp")
    hdr = os.path.join(ROOT, "katome_amd", "csrc", "dist_gfa_dir.h")
    so = os.path.join(HERE, "hostshim", "libdist_gfa_dir_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    for name, args in (("per", 2), ("base", 3), ("range", 3), ("owner", 3), ("address", 3)):
        f = getattr(lib, "hs_gfa_dir_" + name)
        f.restype = C.c_uint64
        f.argtypes = [C.c_uint64, C.c_uint32] + ([C.c_uint64 if name in ("owner", "address") else C.c_uint32] if args == 3 else [])
    return lib


# total_nodes a multiple of world, not a multiple, smaller than world, 0, 1, and sizes past 32 bits
TOTALS = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 1000, 1001, 2 ** 32 - 1, 2 ** 32, 2 ** 40 - 3]


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8, 64])
def test_directory_ranges_tile_the_ids(shim, world):
    for total in TOTALS:
        per, ranges = dm.directory(total, world)
        assert shim.hs_gfa_dir_per(total, world) == per >= 1
        got = [(shim.hs_gfa_dir_base(total, world, r), shim.hs_gfa_dir_range(total, world, r)) for r in range(world)]
        assert got == ranges
        # the ranges follow one another and cover [0, total) exactly; trailing ranks may own nothing
        at = 0
        for base, n in got:
            assert base == at and n <= per
            at += n
        assert at == total
        assert per * world >= total and (total == 0 or per * world - total < world or per == 1)


@pytest.mark.parametrize("world", [1, 3, 8, 64])
def test_owner_is_the_rank_whose_range_holds_the_id(shim, world):
    rng = np.random.default_rng(world)
    for total in TOTALS[1:]:
        per, ranges = dm.directory(total, world)
        ids = {0, total - 1, total // 2} | {int(x) for x in rng.integers(0, total, 20)} | {min(total - 1, r * per) for r in range(world)}
        for v in ids:
            owner = shim.hs_gfa_dir_owner(total, world, v)
            assert owner == v // per < world
            base, n = ranges[owner]
            assert base <= v < base + n
            assert shim.hs_gfa_dir_address(total, world, v) == (owner << 56) | v


# ---- the model's own checks ----------------------------------------------------------------------------------------------------
def _graph(rng, n, n_nodes, k):
    seqs = ["".join(rng.choice(list("ACGT"), int(m))) for m in rng.integers(k, 40, n)]
    kmers = [len(s) - k + 1 for s in seqs]
    return ([int(x) for x in rng.integers(0, n_nodes, n)], [int(x) for x in rng.integers(0, n_nodes, n)],
            [int(x) for x in rng.integers(1, 2 ** 32, n)], kmers, seqs)


@pytest.mark.parametrize("n,n_nodes", [(0, 1), (1, 1), (12, 3), (120, 40)])
def test_numbered_model_from_zero_is_the_plain_model(n, n_nodes):
    k = 5
    src, dst, weight, kmers, seqs = _graph(np.random.default_rng(n), n, n_nodes, k)
    want, seg, first = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)
    link_first, link_b = dm.link_table(src, dst)
    s, l, seg_off = dm.part_text(k, weight, kmers, seqs, 0, True, link_first, link_b)
    assert s + l == want and seg_off == seg and link_first == first
    assert dm.whole_text(k, [(weight, kmers, seqs, link_first, link_b)]) == want


@pytest.mark.parametrize("cuts", [(0,), (5,), (40, 40), (1, 60, 119), (120,)])
def test_parts_put_together_are_the_text_of_the_concatenated_arrays(cuts):
    """the specification in one sentence (include/katome_gpu.h): the ranks' parts, in rank order, are gfa_text of the
    concatenated arrays (empty ranks included)"""
    k, n = 5, 120
    src, dst, weight, kmers, seqs = _graph(np.random.default_rng(7), n, 40, k)
    want, _, _ = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)
    link_first, link_b = dm.link_table(src, dst)
    bounds = [0] + list(cuts) + [n]
    parts = []
    for lo, hi in zip(bounds, bounds[1:]):
        lf = [x - link_first[lo] for x in link_first[lo:hi + 1]]
        parts.append((weight[lo:hi], kmers[lo:hi], seqs[lo:hi], lf, link_b[link_first[lo]:link_first[hi]]))
    assert dm.whole_text(k, parts) == want
    segments, lks = gfa_model.parse(want)
    assert [s[0] for s in segments] == list(range(n)) and [(a, b) for a, b, _ in lks] == gfa_model.links(src, dst)


def test_numbers_of_twenty_digits_and_padding():
    s, l, seg = dm.part_text(5, [3], [2], ["ACGTAC"], 10 ** 19, False, [0, 2], [2 ** 64 - 1, 7])
    assert s == b"S\t10000000000000000000\tACGTAC\tLN:i:6\tKC:i:6\tew:i:3\n" and seg == [23]
    assert l == b"L\t10000000000000000000\t+\t18446744073709551615\t+\t4M\nL\t10000000000000000000\t+\t7\t+\t4M\n"
    assert len(dm.padded(s)) % 16 == 0 and dm.padded(s).rstrip(b"\0") == s and dm.padded(b"") == b""
    assert dm.lines_across_tiles(b"x" * 8185 + b"\nL\t" + b"1" * 20 + b"\t+\t5\t+\t4M\n", 20) == [b"L\t" + b"1" * 20 + b"\t+\t5\t+\t4M"]
