"""katome_amd/csrc/multi_route.h (which way a host build over several GPUs goes) against the rules written out here, for every
combination of flags, request, environment and graph size."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FS, RDP, SHARE = 1, 2, 4                     # KATOME_FLAG_FIRST_SEEN_ORDER, _REMOVE_DEAD_PATHS, _RANKS_SHARE_DEVICE
LIMIT = 0xFFFFFFFF
VALUES = (None, "sharded", "gather", "other")           # unset, the two values that mean something, one that does not
REQUESTS = ("graph", "graph+stages", "contigs")
SIZES = ((LIMIT - 1, LIMIT - 1), (LIMIT, 5), (5, LIMIT))    # below the limit; edges at it; nodes at it


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "hostshim", "multi_route_host.cpp")
    hdr = os.path.join(ROOT, "katome_amd", "csrc", "multi_route.h")
    so = os.path.join(HERE, "hostshim", "libmulti_route_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.hs_multi_route.restype = C.c_uint32
    lib.hs_multi_route.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_uint64, C.c_uint64]
    return lib


def plan(shim, flags, request, totals):
    bits = shim.hs_multi_route(flags, request == "contigs", b"dcw" if request == "graph+stages" else None, *totals)
    names = ("sharded_shrink", "gather_fast", "e_arg", "direct", "gather", "sharded_rdp", "sharded_letters", "local")
    return {n: bool(bits >> i & 1) for i, n in enumerate(names)}


def expected(fs, rdp, request, shrink, prune, dstages, totals):
    """the table of rules, one line each"""
    contigs, stages = request == "contigs", request == "graph+stages"
    want = {}
    want["sharded_shrink"] = contigs and shrink == "sharded"
    want["gather_fast"] = contigs and shrink == "gather"
    want["e_arg"] = not fs and ((contigs and not want["sharded_shrink"]) or stages or rdp)
    want["direct"] = fs and (not contigs or want["sharded_shrink"]) and not stages and prune != "gather"
    gather = fs and not want["direct"]
    if gather and stages:
        too_big = totals[0] >= LIMIT or totals[1] >= LIMIT
        if dstages == "sharded" or (too_big and dstages != "gather"):
            gather = False
    want["gather"] = gather
    # on the sharded graph: remove_dead_paths, then the sharded shrink and nothing further, else the stage letters
    want["sharded_rdp"] = fs and rdp
    want["sharded_letters"] = fs and stages and not want["sharded_shrink"]
    return want


def test_every_combination(shim, monkeypatch):
    cases = 0
    for shrink, prune, dstages in itertools.product(VALUES, repeat=3):
        for name, v in (("KATOME_DIST_SHRINK", shrink), ("KATOME_DIST_PRUNE", prune), ("KATOME_DIST_STAGES", dstages)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        for fs, rdp, request, totals in itertools.product((False, True), (False, True), REQUESTS, SIZES):
            got = plan(shim, (FS if fs else 0) | (RDP if rdp else 0), request, totals)
            want = expected(fs, rdp, request, shrink, prune, dstages, totals)
            assert {k: got[k] for k in want} == want, (fs, rdp, request, shrink, prune, dstages, totals)
            cases += 1
    assert cases == 4 ** 3 * 2 * 2 * 3 * 3


def test_an_empty_stage_string_is_no_stages(shim, monkeypatch):
    for name in ("KATOME_DIST_SHRINK", "KATOME_DIST_PRUNE", "KATOME_DIST_STAGES"):
        monkeypatch.delenv(name, raising=False)
    bits = shim.hs_multi_route(0, 0, b"", 5, 5)
    assert not bits & 4                                  # a packed-key graph with stages = "": no KATOME_E_ARG
    assert shim.hs_multi_route(FS, 0, b"", 5, 5) & 8     # and in first-seen order it goes direct


@pytest.mark.parametrize("comm", VALUES[:1] + ("local", "rccl"))
@pytest.mark.parametrize("share", (False, True))
def test_transport(shim, monkeypatch, comm, share):
    if comm is None:
        monkeypatch.delenv("KATOME_COMM", raising=False)
    else:
        monkeypatch.setenv("KATOME_COMM", comm)
    got = plan(shim, FS | (SHARE if share else 0), "graph", (5, 5))
    assert got["local"] == (share or comm == "local")
