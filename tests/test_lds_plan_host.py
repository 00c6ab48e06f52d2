"""katome_amd/csrc/lds_plan.h (the sizes of the LDS counting tables and the arithmetic that plans a level with them) against the
rules written out here -- runs without a GPU."""
import ctypes as C
import math
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THREADS, MAX_ROUNDS = 1024, 32
# shape -> (slots, fill): the table of the kernels' constants
TABLES = {0: (8192, 5800), 1: (13312, 9425), 2: (5120, 3625), 3: (4096, 4096 // 20 * 11), 4: (7168, 7168 // 20 * 11),
          5: (3072, 3072 // 20 * 11), 6: (5120, 5120 // 20 * 11), 7: (19456, 0)}
LP_SLOTS = 19456


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "hostshim", "lds_plan_host.cpp")
    hdr = os.path.join(ROOT, "katome_amd", "csrc", "lds_plan.h")
    so = os.path.join(HERE, "hostshim", "liblds_plan_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.hs_lds_table.argtypes = [C.c_int, C.POINTER(C.c_uint32)]
    for name, args in (("hs_lc_rounds", [C.c_uint64, C.c_uint32]), ("hs_lc_rounds_try", [C.c_uint64, C.c_double, C.c_uint32]),
                       ("hs_lp_rounds", [C.c_uint64])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_uint32, args
    for name, args in (("hs_lp_group_fits", [C.c_uint64]), ("hs_lf_small_table", [C.c_uint64, C.c_uint32]),
                       ("hs_lc_level_fits", [C.c_uint64, C.c_uint32]), ("hs_lcs_level_fits", [C.c_uint64])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, args
    return lib


def table(shim, shape):
    out = (C.c_uint32 * 2)()
    shim.hs_lds_table(shape, out)
    return out[0], out[1]


def test_table_sizes(shim):
    assert table(shim, 99) == (THREADS, MAX_ROUNDS)
    for shape, want in TABLES.items():
        assert table(shim, shape) == want, shape
    # the 12-byte-slot tables' fill is load 0.71 of the slots: 2900 of every 4096
    for shape, per in ((0, 8), (1, 13), (2, 5)):
        assert TABLES[shape] == (THREADS * per, int(THREADS * per / 4096.0 * 2900))
    assert TABLES[3][1] == 2244 and TABLES[4][1] == 3938 and TABLES[5][1] == 1683 and TABLES[6][1] == 2816


@pytest.mark.parametrize("shape", (0, 1, 2))
def test_sub_rounds(shim, shape):
    """R: a group's share of a sub-round fits even if every record is a new key; R_try: with `optimism` of them taken for distinct;
    R_p: the 8-byte slots at 56 % distinct and load 0.66"""
    fill = TABLES[shape][1]
    for avg in (0, 1, fill, fill + 1, MAX_ROUNDS * fill, MAX_ROUNDS * fill + 1):
        assert shim.hs_lc_rounds(avg, fill) == max(1, -(-avg // fill)), avg
        for optimism in (0.75, 0.05):
            assert shim.hs_lc_rounds_try(avg, optimism, fill) == max(1, math.ceil(avg * optimism / fill)), (avg, optimism)
        assert shim.hs_lp_rounds(avg) == max(1, math.ceil(avg * 0.56 / (LP_SLOTS * 0.66))), avg
    assert shim.hs_lc_rounds(MAX_ROUNDS * fill, fill) == MAX_ROUNDS and shim.hs_lc_rounds(MAX_ROUNDS * fill + 1, fill) == MAX_ROUNDS + 1
    # what a level may hold: 2^16 groups of MAX_ROUNDS sub-rounds
    top = (MAX_ROUNDS * fill) << 16
    assert shim.hs_lc_level_fits(top + 0xFFFF, fill) and not shim.hs_lc_level_fits(top + 0x10000, fill)


def test_first_seen_level_bound(shim):
    fill = TABLES[2][1]
    assert MAX_ROUNDS * fill << 16 >= 1 << 32              # (so the 32-bit record positions are what binds)
    assert shim.hs_lcs_level_fits((1 << 32) - 1) and not shim.hs_lcs_level_fits(1 << 32)


def test_packed_fit_boundary(shim):
    """a group goes through the 8-byte slots in one visit while avg * 0.56 <= LP_SLOTS * 0.66"""
    edge = int(LP_SLOTS * 0.66 / 0.56)                     # 22930: the last avg on the fitting side
    assert edge * 0.56 <= LP_SLOTS * 0.66 < (edge + 1) * 0.56
    assert shim.hs_lp_group_fits(edge) and not shim.hs_lp_group_fits(edge + 1)
    assert shim.hs_lp_group_fits(0)
    assert shim.hs_lp_rounds(edge) == 1 and shim.hs_lp_rounds(edge + 1) == 2


@pytest.mark.parametrize("small_shape", (3, 5))
def test_whole_key_table_choice(shim, small_shape):
    """the small whole-key table while a group's distinct keys leave it a third full: SLOTS(small) / 20 * 7, for both key widths"""
    slots = TABLES[small_shape][0]
    edge = slots // 20 * 7
    assert edge == {3: 1428, 5: 1071}[small_shape]
    assert shim.hs_lf_small_table(edge, slots) and not shim.hs_lf_small_table(edge + 1, slots)
    assert shim.hs_lf_small_table(0, slots)
