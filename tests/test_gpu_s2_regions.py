"""S2 of the ordered k-mer count written by its first partition digit (lds_count_ordered_kernel with REGIONS, KATOME_S2_REGIONS): 256
regions with a cursor each instead of one cursor, and one partition pass over them (radix.hip, RegionSource) instead of two over a
dense S2.  The pass alone is checked against numpy through katome_dev_s2_region_pass.  Whole builds must give byte for byte the
arrays of the route without regions (KATOME_S2_REGIONS=0) and of the full edge sort (KATOME_EDGE_HALF_SORT=0), also on the way back
when a region fills (KATOME_S2_REGION_CAP).  The switches are read once, so every route runs in a process of its own, side by side."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096


# ---- the pass alone ---------------------------------------------------------------------------------------------------------------------
def _used_cases():
    cases = {"one_key_each": [1] * 256, "all_empty": [0] * 256}
    for u in (4095, 4096, 4097, 8192):
        used = [0] * 256
        used[37] = u
        cases["one_region_%d" % u] = used
    used = [0] * 256
    used[0], used[255] = 5000, 4097
    cases["first_and_last"] = used
    rng = np.random.default_rng(3)
    cases["three_tiles_each"] = [int(x) for x in rng.integers(2 * TILE + 1, 3 * TILE + 1, 256)]
    return cases


_USED = _used_cases()


@pytest.mark.parametrize("k", (31, 11))
@pytest.mark.parametrize("case", sorted(_USED))
def test_the_pass_alone_equals_a_stable_partition_by_the_top_byte(case, k):
    """keys and weights laid out in regions (the unused rest of every region and of the byte stream filled with 0xFF) -> numpy's
    stable partition by key >> (2k - 8) of the regions read in digit order"""
    import torch
    from katome_amd import device as kd
    used = _USED[case]
    start = [int(x) for x in kd.s2_region_starts(used)]
    assert start[0] == 0 and all(start[d + 1] - start[d] == (used[d] + TILE - 1) // TILE * TILE for d in range(256))
    rng = np.random.default_rng(1000 * k + len(case))
    total = max(start[256], 1)
    keys = np.full(total, 0xFFFFFFFFFFFFFFFF, np.uint64)
    wts = np.full(total, 0xFFFFFFFF, np.uint32)
    digits = np.full(total, 0xFF, np.uint8)
    low_bits = 2 * k - 16
    dense_k, dense_w = [], []
    for d in range(256):
        u = used[d]
        if not u:
            continue
        top = rng.integers(0, 256, u, dtype=np.uint64)
        if d % 3 == 0:
            top[:] = top[0]                                                 # (a region that is one run of the second digit)
        kk = (top << np.uint64(low_bits + 8)) | (np.uint64(d) << np.uint64(low_bits)) | rng.integers(0, 1 << low_bits, u, dtype=np.uint64)
        ww = rng.integers(1, 1 << 16, u, dtype=np.uint32)
        keys[start[d]:start[d] + u], wts[start[d]:start[d] + u] = kk, ww
        digits[start[d]:start[d] + u] = (kk >> np.uint64(2 * k - 8)).astype(np.uint8)
        dense_k.append(kk)
        dense_w.append(ww)
    n = sum(used)
    out_k, out_w = kd.s2_region_pass(k, used, torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(wts.view(np.int32)).cuda(),
                                     torch.from_numpy(digits).cuda())
    assert out_k.numel() == out_w.numel() == n
    if not n:
        return
    dense_k, dense_w = np.concatenate(dense_k), np.concatenate(dense_w)
    order = np.argsort(dense_k >> np.uint64(2 * k - 8), kind="stable")
    assert out_k.cpu().numpy().view(np.uint64).tobytes() == dense_k[order].tobytes()
    assert out_w.cpu().numpy().view(np.uint32).tobytes() == dense_w[order].tobytes()


# ---- whole small builds -----------------------------------------------------------------------------------------------------------------
_SCRIPT = r"""
import sys, hashlib, random, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii, kmer_to_int
from oracle import oracle as o
from katome_amd import device as kd
from katome_amd.build import GpuGraph

COMP = str.maketrans("ACGT", "TGCA")

def crowded(seed, n):
    # tests/test_gpu_lds_order.py: n reads A x 8 + 15 bases + T x 8 + 29 of C, G -- n 31-mers of group 0 whose reverse complements begin
    # with A x 8 as well, so that one group holds them and ONE region takes all of its S2
    rng = random.Random(seed)
    seen, reads = set(), []
    while len(reads) < n:
        mid = "".join(rng.choice("ACGT") for _ in range(15))
        if mid[0] == "A" or mid[-1] == "T" or "A" * 8 in mid or "T" * 8 in mid:
            continue
        r = "A" * 8 + mid + "T" * 8
        rc = r.translate(COMP)[::-1]
        if r in seen or rc in seen:
            continue
        seen.add(r)
        reads.append(r + "".join(rng.choice("CG") for _ in range(29)))
    return np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in reads])

def digest(name, reads, k, rc=True, min_weight=0):
    print("CASE", name, file=sys.stderr, flush=True)
    L = reads.shape[1]
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, rc)
    if min_weight:
        b.remove_weak_edges(min_weight)
    b.count_reads(packed, len(reads), L, None, first_read=0)
    dg = b.finalize()
    h = hashlib.sha256()
    for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
        h.update(t.cpu().numpy().tobytes())
    print("RG", name, dg.n_nodes, dg.n_edges, h.hexdigest(), flush=True)
    b.close()

for k in range(11, 33, 2):
    digest("k%d" % k, o.synth_reads(k, 4000, 150, 30000, 3e-3, 0), k)
digest("min_weight", o.synth_reads(5, 4000, 150, 20000, 3e-3, 0), 31, True, 3)
digest("reads_101", o.synth_reads(6, 4000, 101, 30000, 3e-3, 0), 31)
digest("one_strand", o.synth_reads(3, 3000, 150, 30000, 3e-3, 0), 31, False)
for n in (4095, 4097, 14000, 17000):
    digest("crowded_%d" % n, crowded(n, n), 31)
print("CASE oracle", file=sys.stderr, flush=True)
k = 31
reads = o.synth_reads(7, 3000, 150, 25000, 3e-3, 0)
g, rb = GpuGraph.create_from_packed(pack_reads_ascii(reads).reshape(-1), len(reads), reads.shape[1], reverse_complement=True, k=k)
ref = o.build_ascii(reads, k, True)
assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges), (g.n_nodes, g.n_edges, ref.n_nodes, ref.n_edges)
assert g.key_ints("edge") == sorted(kmer_to_int(s) for s in ref.kmer_strings())
assert g.multiset() == ref.multiset()
print("RG oracle", g.n_nodes, g.n_edges, "ORACLE_OK", flush=True)
"""

_TWO_STRANDS = ["k%d" % k for k in range(11, 33, 2)] + ["min_weight", "reads_101", "crowded_4095", "crowded_4097", "crowded_14000", "crowded_17000", "oracle"]
_CASES = _TWO_STRANDS + ["one_strand"]
_ROUTES = {"regions": {"KATOME_S2_REGIONS": "2"}, "no_regions": {"KATOME_S2_REGIONS": "0"}, "edge_sort": {"KATOME_EDGE_HALF_SORT": "0"},
           "way_back": {"KATOME_S2_REGIONS": "2", "KATOME_S2_REGION_CAP": "64"}, "default": {}}
_ONE_PASS = "one pass, counted from its writer's digits"
_REBUILT = "rebuilt from S1"
_FULL = "too large for the merge's LDS; sorted in full"


@pytest.fixture(scope="module")
def routes():
    """route -> (case -> its RG row, case -> the trace lines of its build); the five processes run side by side"""
    env = {name: dict(os.environ, KATOME_SORTED_COUNT="2", KATOME_LC_TRACE="1", **extra) for name, extra in _ROUTES.items()}
    env["default"].pop("KATOME_S2_REGIONS", None)          # (whatever the caller's environment says: the default is what is asked)
    procs = {name: subprocess.Popen([sys.executable, "-c", _SCRIPT, ROOT], env=env[name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for name in _ROUTES}
    res = {}
    try:
        for name, p in procs.items():
            out, err = p.communicate(timeout=600)
            assert p.returncode == 0, (name, err[-3000:])
            rows = {line.split()[1]: line for line in out.splitlines() if line.startswith("RG ")}
            trace, case = {}, None
            for line in err.splitlines():
                if line.startswith("CASE "):
                    case = line.split()[1]
                    trace[case] = []
                elif case is not None:
                    trace[case].append(line)
            res[name] = (rows, trace)
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    return res


def _count(lines, what):
    return sum(what in line for line in lines)


@pytest.mark.parametrize("case", _CASES)
def test_every_route_gives_the_same_arrays(routes, case):
    rows = routes["regions"][0]
    assert case in rows
    for name in _ROUTES:
        assert routes[name][0].get(case) == rows[case], (name, case)
    assert "ORACLE_OK" in routes["regions"][0]["oracle"]


@pytest.mark.parametrize("case", _TWO_STRANDS)
def test_the_regions_route_runs_one_pass_over_s2(routes, case):
    """the new trace line, no way back, the largest-group line as before, and one `[order] by key:` line fewer than without regions
    (the records' own order stays; S2 has none)"""
    lines, plain = routes["regions"][1][case], routes["no_regions"][1][case]
    assert _count(lines, _ONE_PASS) == 1 and _count(lines, _REBUILT) == 0, lines
    assert _count(lines, "[half sort] S2: ") == 1, lines
    assert _count(plain, "S2 regions") == 0, plain
    assert _count(lines, "[order] by key:") == _count(plain, "[order] by key:") - 1, (lines, plain)


def test_one_strand_has_no_s2_and_takes_no_regions(routes):
    lines = routes["regions"][1]["one_strand"]
    assert _count(lines, "[lds count] in key order") == 1 and _count(lines, "S2 regions") == 0, lines


def test_the_largest_crowded_group_goes_on_to_the_full_s2_sort(routes):
    for name in ("regions", "way_back"):
        assert _count(routes[name][1]["crowded_17000"], _FULL) == 1, routes[name][1]["crowded_17000"]
    assert _count(routes["regions"][1]["crowded_14000"], _FULL) == 0


@pytest.mark.parametrize("case", _TWO_STRANDS)
def test_a_full_region_is_rebuilt_from_s1(routes, case):
    """64 keys to a region: every build here overflows one, S2 is made again from S1 and takes the two passes it took before"""
    lines, plain = routes["way_back"][1][case], routes["no_regions"][1][case]
    assert _count(lines, _REBUILT) == 1 and _count(lines, _ONE_PASS) == 0, lines
    assert _count(lines, "[order] by key:") == _count(plain, "[order] by key:"), (lines, plain)


def test_a_small_build_takes_no_regions_by_default(routes):
    for case in _CASES:
        assert _count(routes["default"][1][case], "S2 regions") == 0, case
