"""katome_amd/csrc/s2_regions.h (the 256 regions that S2 of the ordered k-mer count is written into, one per first partition digit)
against the rules written out here -- runs without a GPU.

  sample        every 256-record row of a level below 2^22 records, else every 32nd row: never fewer than n / 64 records
  cap[d]        min(n, est + est // 16 + 4096) rounded up to 4096-key tiles, est = counts[d] * n // sampled
  start         the caps' prefix sums: ascending, disjoint, tile-aligned
  logical tiles region d contributes ceil(used[d] / 4096) of them, in digit order, the last one partial, none when empty
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostshim", "s2_regions_host.cpp")
HDR = os.path.join(ROOT, "katome_amd", "csrc", "s2_regions.h")
TILE = 4096
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "hostshim", "libs2_regions_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.hs_s2_sample.restype, lib.hs_s2_sample.argtypes = None, [C.c_uint64, u64p, u64p, u64p]
    lib.hs_s2_caps.restype, lib.hs_s2_caps.argtypes = None, [u32p, C.c_uint64, C.c_uint64, u64p]
    lib.hs_s2_starts.restype, lib.hs_s2_starts.argtypes = None, [u64p, u64p]
    lib.hs_s2_tiles.restype, lib.hs_s2_tiles.argtypes = None, [u64p, u32p]
    lib.hs_s2_tile.restype, lib.hs_s2_tile.argtypes = None, [C.c_uint32, u32p, u64p, u64p, u32p, u64p, u32p]
    return lib


def sample(shim, n):
    rows, stride, rec = C.c_uint64(), C.c_uint64(), C.c_uint64()
    shim.hs_s2_sample(n, C.byref(rows), C.byref(stride), C.byref(rec))
    return rows.value, stride.value, rec.value


def caps(shim, counts, sampled, n):
    c = np.ascontiguousarray(counts, np.uint32)
    cap = np.zeros(256, np.uint64)
    shim.hs_s2_caps(c.ctypes.data_as(u32p), sampled, n, cap.ctypes.data_as(u64p))
    return [int(x) for x in cap]


def starts(shim, cap):
    c = np.ascontiguousarray(cap, np.uint64)
    st = np.zeros(257, np.uint64)
    shim.hs_s2_starts(c.ctypes.data_as(u64p), st.ctypes.data_as(u64p))
    return [int(x) for x in st]


def tiles(shim, used):
    u = np.ascontiguousarray(used, np.uint64)
    first = np.zeros(257, np.uint32)
    shim.hs_s2_tiles(u.ctypes.data_as(u64p), first.ctypes.data_as(u32p))
    return [int(x) for x in first]


def tile(shim, t, first, start, used):
    f, s, u = np.ascontiguousarray(first, np.uint32), np.ascontiguousarray(start, np.uint64), np.ascontiguousarray(used, np.uint64)
    region, at, keys = C.c_uint32(), C.c_uint64(), C.c_uint32()
    shim.hs_s2_tile(t, f.ctypes.data_as(u32p), s.ctypes.data_as(u64p), u.ctypes.data_as(u64p), C.byref(region), C.byref(at), C.byref(keys))
    return region.value, at.value, keys.value


def test_the_sample_reads_every_record_of_a_small_level_and_a_64th_at_least_of_a_large_one(shim):
    for n in (0, 1, 255, 256, 257, 4000, (1 << 22) - 1):
        rows, stride, rec = sample(shim, n)
        assert stride == 1 and rec == n and rows == (n + 255) // 256
    for n in (1 << 22, (1 << 22) + 1, (1 << 22) + 8191, (1 << 22) + 8192, 10 ** 7 + 3, 1450000000, (1 << 33) + 77):
        rows, stride, rec = sample(shim, n)
        assert stride == 32
        first = [r * stride * 256 for r in (0, rows - 1)]
        assert first[1] < n <= first[1] + stride * 256                    # (evenly spread: the last sampled row lies in the last stride)
        assert rec == (rows - 1) * 256 + min(256, n - first[1])
        assert rec * 64 >= n


def test_caps_bound_the_exact_counts_when_the_sample_is_the_whole_level(shim):
    rng = random.Random(22)
    for n_target in (1, 300, 5000, 100000, (1 << 22) - 1):
        for shape in ("even", "one", "skewed"):
            if shape == "even":
                counts = [n_target // 256 + (1 if d < n_target % 256 else 0) for d in range(256)]
            elif shape == "one":
                counts = [0] * 256
                counts[rng.randrange(256)] = n_target
            else:
                cuts = sorted(rng.randrange(n_target + 1) for _ in range(255))
                counts = [b - a for a, b in zip([0] + cuts, cuts + [n_target])]
            n = sum(counts)
            assert n == n_target
            cap = caps(shim, counts, n, n)
            for d in range(256):
                assert cap[d] >= counts[d] and cap[d] % TILE == 0
                assert cap[d] == (min(n, counts[d] + counts[d] // 16 + 4096) + TILE - 1) // TILE * TILE


def test_caps_scale_a_sample_and_stay_within_the_levels_room(shim):
    rng = random.Random(23)
    for n in (1 << 22, 10 ** 7 + 3, 1450000000, (1 << 33) + 77):
        _, _, rec = sample(shim, n)
        cuts = sorted(rng.randrange(rec + 1) for _ in range(255))
        counts = [b - a for a, b in zip([0] + cuts, cuts + [rec])]
        cap = caps(shim, counts, rec, n)
        for d in range(256):
            est = counts[d] * n // rec
            assert cap[d] == (min(n, est + est // 16 + 4096) + TILE - 1) // TILE * TILE
        # the regions exceed the n + 1 keys of one cursor's S2 by n / 16 + 512 tiles at most
        assert sum(cap) <= n + 1 + n // 16 + 512 * TILE


def test_starts_are_ascending_disjoint_and_tile_aligned(shim):
    rng = random.Random(24)
    cap = [rng.randrange(1, 50) * TILE for _ in range(256)]
    st = starts(shim, cap)
    assert st[0] == 0 and st[256] == sum(cap)
    for d in range(256):
        assert st[d] % TILE == 0 and st[d + 1] - st[d] == cap[d] and st[d + 1] > st[d]


def _check_tiles(shim, used):
    cap = [max(1, (u + TILE - 1) // TILE) * TILE for u in used]
    st = starts(shim, cap)
    first = tiles(shim, used)
    assert first[0] == 0
    for d in range(256):
        assert first[d + 1] - first[d] == (used[d] + TILE - 1) // TILE
    assert first[256] == sum((u + TILE - 1) // TILE for u in used)
    t = 0
    for d in range(256):                                                   # digit order, the last tile of a region partial, none when empty
        left = used[d]
        while left:
            assert tile(shim, t, first, st, used) == (d, st[d] + used[d] - left, min(left, TILE)), (t, d)
            left -= min(left, TILE)
            t += 1
    assert t == first[256]


@pytest.mark.parametrize("u", (0, 1, 4095, 4096, 4097, 8192))
def test_the_logical_tiles_of_one_region_among_empty_ones(shim, u):
    for d in (0, 1, 100, 255):
        used = [0] * 256
        used[d] = u
        _check_tiles(shim, used)


def test_the_logical_tiles_of_mixed_regions(shim):
    _check_tiles(shim, [0] * 256)
    _check_tiles(shim, [1] * 256)
    edge = (0, 1, 4095, 4096, 4097, 8192)
    _check_tiles(shim, [edge[d % 6] for d in range(256)])
    _check_tiles(shim, [edge[(d * 7 + 3) % 6] for d in range(256)])
    used = [0] * 256
    used[0], used[255] = 4097, 1
    _check_tiles(shim, used)


def _run(exe, env=None):
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    word, checks = out.stdout.split()
    with open(SRC) as f:
        written = f.read().count("\n    CHECK(")
    assert word == "ok" and int(checks) == written >= 15           # (every check the program holds was reached)


def test_pins_as_a_program(tmp_path):
    exe = str(tmp_path / "s2_regions_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe])
    _run(exe)


def test_pins_under_asan_and_ubsan(tmp_path):
    probe = tmp_path / "t.c"
    probe.write_text("int main(void){return 0;}\n")
    try:
        subprocess.check_call(["gcc"] + SAN + [str(probe), "-o", str(tmp_path / "t")], stderr=subprocess.DEVNULL)
        have = subprocess.call([str(tmp_path / "t")], env=ENV) == 0
    except (subprocess.CalledProcessError, OSError):
        have = False
    if not have:
        pytest.skip("gcc sanitizer runtime not available")
    exe = str(tmp_path / "s2_regions_host_san")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + [SRC, "-o", exe])
    _run(exe, ENV)
