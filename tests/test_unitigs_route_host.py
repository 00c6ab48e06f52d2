"""katome_amd/csrc/multi_route.h with `unitigs` (the route of katome_unitigs_* over several GPUs): never a gather, KATOME_E_ARG
exactly when stage letters or remove_dead_paths come without first-seen order, whatever the environment; and without `unitigs`
every bit of every combination is what the plan was before the parameter existed."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FS, RDP, SHARE = 1, 2, 4
LIMIT = 0xFFFFFFFF
VALUES = (None, "sharded", "gather", "other")
SIZES = ((5, 5), (LIMIT - 1, LIMIT - 1), (LIMIT, 5), (5, LIMIT), (2 ** 40, 2 ** 40))
NAMES = ("sharded_shrink", "gather_fast", "e_arg", "direct", "gather", "sharded_rdp", "sharded_letters", "local", "unitigs")


def _build(name):
    src = os.path.join(HERE, "hostshim", name + ".cpp")
    hdr = os.path.join(ROOT, "katome_amd", "csrc", "multi_route.h")
    so = os.path.join(HERE, "hostshim", "lib%s.so" % name)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def shims():
    new, old = _build("unitigs_route_host"), _build("multi_route_host")     # (the second: compiled WITHOUT naming the new parameter)
    new.hs_unitigs_route.restype = C.c_uint32
    new.hs_unitigs_route.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_int, C.c_uint64, C.c_uint64]
    old.hs_multi_route.restype = C.c_uint32
    old.hs_multi_route.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_uint64, C.c_uint64]
    return new, old


def _environments(monkeypatch):
    for shrink, prune, dstages in itertools.product(VALUES, repeat=3):
        for name, v in (("KATOME_DIST_SHRINK", shrink), ("KATOME_DIST_PRUNE", prune), ("KATOME_DIST_STAGES", dstages)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        yield shrink, prune, dstages


def test_unitigs_never_gather(shims, monkeypatch):
    new, _ = shims
    monkeypatch.delenv("KATOME_COMM", raising=False)
    cases = 0
    for env in _environments(monkeypatch):
        for fs, rdp, share, stages, totals in itertools.product((False, True), (False, True), (False, True), (None, b"", b"dcwced", b"d"), SIZES):
            flags = (FS if fs else 0) | (RDP if rdp else 0) | (SHARE if share else 0)
            for want_contigs in (0, 1):                  # (the entries pass false; the flag wins either way)
                bits = new.hs_unitigs_route(flags, want_contigs, stages, 1, *totals)
                got = {n: bool(bits >> i & 1) for i, n in enumerate(NAMES)}
                letters = bool(stages)
                want = dict(sharded_shrink=False, gather_fast=False, e_arg=(not fs) and (letters or rdp), direct=False, gather=False,
                            sharded_rdp=fs and rdp, sharded_letters=fs and letters, local=share, unitigs=True)
                assert got == want, (env, fs, rdp, share, stages, totals)
                cases += 1
    assert cases == 4 ** 3 * 2 * 2 * 2 * 4 * len(SIZES) * 2


def test_without_the_flag_nothing_changes(shims, monkeypatch):
    new, old = shims
    monkeypatch.delenv("KATOME_COMM", raising=False)
    cases = 0
    for env in _environments(monkeypatch):
        for flags, want_contigs, stages, totals in itertools.product(range(8), (0, 1), (None, b"", b"dcw"), SIZES):
            assert new.hs_unitigs_route(flags, want_contigs, stages, 0, *totals) == old.hs_multi_route(flags, want_contigs, stages, *totals), \
                (env, flags, want_contigs, stages, totals)
            cases += 1
    assert cases == 4 ** 3 * 8 * 2 * 3 * len(SIZES)


@pytest.mark.parametrize("comm", (None, "local", "rccl"))
def test_transport(shims, monkeypatch, comm):
    new, _ = shims
    if comm is None:
        monkeypatch.delenv("KATOME_COMM", raising=False)
    else:
        monkeypatch.setenv("KATOME_COMM", comm)
    for share in (False, True):
        bits = new.hs_unitigs_route(FS | (SHARE if share else 0), 0, b"dcwced", 1, 5, 5)
        assert bool(bits & 128) == (share or comm == "local")
