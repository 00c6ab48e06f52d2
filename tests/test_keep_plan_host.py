"""katome_amd/csrc/keep_plan.h (grow, keep or refuse for the records a build keeps aside between batches: the big-tile records and
the left-over windows) against the two rules written out here -- runs without a GPU.  With w the words of a record, free what the
driver reports, pool what the library's pool holds idle:

                     tile records                                             left-over windows
  no growth          n + n_new <= cap                                         the same
  want               max(2 cap if cap else 16 n_new, n + n_new)               max(n + n_new, 2 cap)
  refuse             n + n_new > limit, or want 8w 3 > free + pool + cap 8w,  (want + n) 8w > free / 2 (the driver's free only),
                     or want 8w > total / 6                                   or want 8w > total / 8
  limit              KATOME_TILE_RECS_LIMIT, else none                        none
  allocation fails   refuse                                                   the error
  first record set   exact while n == 0                                       never exact
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostshim", "keep_plan_host.cpp")
HDR = os.path.join(ROOT, "katome_amd", "csrc", "keep_plan.h")
TILES, REST = 0, 1
AS_IS, GROW, REFUSE = 0, 1, 2
NONE = 2 ** 64 - 1
GiB = 1 << 30
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "hostshim", "libkeep_plan_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.hs_keep_plan.restype = C.c_int
    lib.hs_keep_plan.argtypes = [C.c_int] + [C.c_uint64] * 3 + [C.c_uint32] + [C.c_uint64] * 4 + [C.POINTER(C.c_uint64)]
    lib.hs_keep_policy_bits.restype, lib.hs_keep_policy_bits.argtypes = C.c_int, [C.c_int]
    return lib


def plan(shim, which, n, cap, n_new, w, free, pool, total, limit):
    want = C.c_uint64(0)
    action = shim.hs_keep_plan(which, n, cap, n_new, w, free, pool, total, limit, C.byref(want))
    return action, want.value


def want_of(which, n, cap, n_new):
    if which == TILES:
        return max(2 * cap if cap else 16 * n_new, n + n_new)
    return max(n + n_new, 2 * cap)


def rule(which, n, cap, n_new, w, free, pool, total, limit):
    """the table above, line by line"""
    if n + n_new <= cap:
        return AS_IS, cap
    want = want_of(which, n, cap, n_new)
    if which == TILES:
        refuse = n + n_new > limit or want * 8 * w * 3 > free + pool + cap * 8 * w or want * 8 * w > total // 6
    else:
        refuse = (want + n) * 8 * w > free // 2 or want * 8 * w > total // 8
    return (REFUSE, 0) if refuse else (GROW, want)


# (n, cap, n_new): nothing kept yet; a full array; room for exactly, one fewer and one more than the batch; a batch beyond the doubling
STATES = [(0, 0, 100), (0, 0, 1), (1600, 1600, 100), (1500, 1600, 100), (1500, 1600, 99), (1500, 1600, 101), (1600, 1600, 5000),
          (100, 100, 100), (200, 200, 100), (37, 64, 28), (3 << 30, 4 << 30, 2 << 30)]


@pytest.mark.parametrize("which", (TILES, REST))
def test_against_the_rule_on_a_grid(shim, which):
    """every inequality of the rule at equality and one off on both sides, the others far from theirs"""
    checked = 0
    for (n, cap, n_new), w in itertools.product(STATES, (1, 2, 3, 4)):
        want = want_of(which, n, cap, n_new)
        rec = 8 * w
        if which == TILES:
            mem_edge = max(want * rec * 3 - cap * rec, 0)      # free + pool at which the memory test turns
            frees = [(mem_edge + d, 0) for d in (-1, 0, 1) if mem_edge + d >= 0]
            frees += [(mem_edge // 2, mem_edge - mem_edge // 2 + d) for d in (-1, 0, 1) if mem_edge - mem_edge // 2 + d >= 0]
            total_edge = want * rec * 6
        else:
            mem_edge = (want + n) * rec * 2
            frees = [(mem_edge + d, p) for d in (-2, -1, 0, 1) for p in (0, 200 * GiB)]
            total_edge = want * rec * 8
        far_free, far_total = (max(mem_edge, 1) * 4, 0), total_edge * 4
        limits = [n + n_new - 1, n + n_new, n + n_new + 1, NONE]
        cases = [(f, far_total, NONE) for f in frees]
        cases += [(far_free, total_edge + d, NONE) for d in (-1, 0, 1, 5, 6, 7, 8)]
        cases += [(far_free, far_total, lim) for lim in limits]
        cases += [(f, total_edge + d, lim) for f in frees for d in (-1, 0) for lim in limits[:2]]
        for (free, pool), total, limit in cases:
            args = (which, n, cap, n_new, w, free, pool, total, limit)
            assert plan(shim, *args) == rule(*args), args
            checked += 1
    assert checked > 1000


def test_both_outcomes_on_each_side_of_every_edge(shim):
    """(the grid above compares two implementations; here the edges themselves, so that neither can be vacuous)"""
    for which in (TILES, REST):
        n, cap, n_new, w = 200, 200, 100, 2
        want = want_of(which, n, cap, n_new)
        assert want == 400
        if which == TILES:
            edge = want * 16 * 3 - cap * 16
            assert plan(shim, which, n, cap, n_new, w, edge, 0, 288 * GiB, NONE) == (GROW, want)
            assert plan(shim, which, n, cap, n_new, w, edge - 1, 0, 288 * GiB, NONE) == (REFUSE, 0)
        else:
            edge = (want + n) * 16 * 2
            assert plan(shim, which, n, cap, n_new, w, edge, 0, 288 * GiB, NONE) == (GROW, want)
            assert plan(shim, which, n, cap, n_new, w, edge - 1, 0, 288 * GiB, NONE) == (REFUSE, 0)


def test_pins(shim):
    big = (200 * GiB, 0, 288 * GiB, NONE)
    # tile set: sixteen batches first, then doubling
    assert plan(shim, TILES, 0, 0, 100, 2, *big) == (GROW, 1600)
    assert plan(shim, TILES, 1600, 1600, 100, 2, *big) == (GROW, 3200)
    # ... the limit: 9001 records handed over against 9000
    assert plan(shim, TILES, 8000, 8000, 1001, 2, 200 * GiB, 0, 288 * GiB, 9000) == (REFUSE, 0)
    assert plan(shim, TILES, 8000, 8000, 1000, 2, 200 * GiB, 0, 288 * GiB, 9000) == (GROW, 16000)
    # ... a pool large enough turns a refusal into growth: 3 x 1600 x 16 bytes are wanted
    assert plan(shim, TILES, 0, 0, 100, 2, 1000, 0, 288 * GiB, NONE) == (REFUSE, 0)
    assert plan(shim, TILES, 0, 0, 100, 2, 1000, 75800, 288 * GiB, NONE) == (GROW, 1600)
    assert plan(shim, TILES, 0, 0, 100, 2, 1000, 75799, 288 * GiB, NONE) == (REFUSE, 0)
    # rest set: what is needed, then doubling
    assert plan(shim, REST, 0, 0, 100, 1, *big) == (GROW, 100)
    assert plan(shim, REST, 100, 100, 100, 1, *big) == (GROW, 200)
    assert plan(shim, REST, 200, 200, 100, 1, *big) == (GROW, 400)
    # ... the same pool makes no difference, and neither does a limit
    assert plan(shim, REST, 0, 0, 100, 1, 1000, 0, 288 * GiB, NONE) == (REFUSE, 0)
    assert plan(shim, REST, 0, 0, 100, 1, 1000, 75800, 288 * GiB, NONE) == (REFUSE, 0)
    assert plan(shim, REST, 0, 0, 100, 1, 1600, 75800, 288 * GiB, 0) == (GROW, 100)
    # want x 8w exactly total / 6 (tiles) and total / 8 (rest): allowed; one byte more than the share: refused
    assert plan(shim, TILES, 0, 0, 100, 2, 200 * GiB, 0, 6 * 1600 * 16, NONE) == (GROW, 1600)
    assert plan(shim, TILES, 0, 0, 100, 2, 200 * GiB, 0, 6 * 1600 * 16 - 1, NONE) == (REFUSE, 0)
    assert plan(shim, REST, 0, 0, 100, 1, 200 * GiB, 0, 8 * 100 * 8, NONE) == (GROW, 100)
    assert plan(shim, REST, 0, 0, 100, 1, 200 * GiB, 0, 8 * 100 * 8 - 1, NONE) == (REFUSE, 0)
    # a failed allocation refuses on the tile set and is an error on the rest set; only the tile set starts out exact
    assert shim.hs_keep_policy_bits(TILES) == 3 and shim.hs_keep_policy_bits(REST) == 0


def _run(exe, env=None):
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    word, checks = out.stdout.split()
    with open(SRC) as f:
        written = f.read().count("\n    CHECK(")
    assert word == "ok" and int(checks) == written >= 19           # (every check the program holds was reached)


def test_pins_as_a_program(tmp_path):
    exe = str(tmp_path / "keep_plan_host")
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
    exe = str(tmp_path / "keep_plan_host_san")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + [SRC, "-o", exe])
    _run(exe, ENV)
