"""The ordering of one 16-bit key group in LDS (lds_order.h) inside the ordered count (lds_count_ordered_kernel) and the merge of the
reverse-complement groups (group_merge_kernel), with groups as full as the headline build's and fuller.  The ordinary small builds
leave a handful of keys per group, so here one group is crowded on purpose: a read begins with A x 8 + 15 bases + T x 8, a 31-mer that
begins with A x 8 and so does its reverse complement -- group 0 takes N representatives (S1) and N reverse complements (S2) from N
reads.  (A read of one window is not counted by sorting at all, so 29 bases of C and G follow: 30 windows, a tile; the middle
neither begins with A, nor ends with T, nor holds a run of eight A's or T's, so none of the other windows or their reverse
complements begins with A x 8 -- they scatter over other groups.)  Every route must give byte for byte the same arrays: the default
one, the full S2 sort (KATOME_S2_GROUP_SORT=0), the full edge sort (KATOME_EDGE_HALF_SORT=0) and the way back through the capacity
hook (KATOME_S2_GROUP_CAP=1); one crowded case is compared with the oracle as well.  The switches are read once, so every route runs
in a process of its own."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_COMMON = r"""
import sys, hashlib, random, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii, kmer_to_int
from oracle import oracle as o
from katome_amd import device as kd

COMP = str.maketrans("ACGT", "TGCA")

def crowded(seed, n, fixed="", first_free="ACGT"):
    # n reads A x 8 + fixed + random bases + T x 8 (no two of these 31-mers the same or each other's reverse complement) + 29 of C, G;
    # the first random base is one of first_free
    rng = random.Random(seed)
    free = 15 - len(fixed)
    seen, reads = set(), []
    while len(reads) < n:
        mid = fixed + rng.choice(first_free) + "".join(rng.choice("ACGT") for _ in range(free - 1))
        if mid[0] == "A" or mid[-1] == "T" or "A" * 8 in mid or "T" * 8 in mid:
            continue
        r = "A" * 8 + mid + "T" * 8
        rc = r.translate(COMP)[::-1]
        if r in seen or rc in seen:
            continue
        seen.add(r)
        reads.append(r + "".join(rng.choice("CG") for _ in range(29)))
    return reads

def as_rows(reads):
    return np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in reads])
"""

_DIGEST_SCRIPT = _COMMON + r"""
def digest(name, reads, k, min_weight=0):
    print("CASE", name, file=sys.stderr, flush=True)
    L = reads.shape[1]
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, True)
    if min_weight:
        b.remove_weak_edges(min_weight)
    b.count_reads(packed, len(reads), L, None, first_read=0)
    dg = b.finalize()
    h = hashlib.sha256()
    for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
        h.update(t.cpu().numpy().tobytes())
    print("LO", name, dg.n_nodes, dg.n_edges, h.hexdigest(), flush=True)
    b.close()

for name, n in (("one_step", 1000), ("several_steps", 3000), ("ring_wrap", 9000), ("large_group", 14000), ("over_the_cap", 17000),
                ("past_the_tail", 18000)):
    digest(name, as_rows(crowded(n, n)), 31)
# A x 8 + C x 7 + 8 bases + T x 8: the remainder's top 14 bits are the same in every such key, so one bucket holds them all, however
# many buckets there are.  The reverse complement, A x 8 + 8 bases + G x 7 + T x 8, spreads over the buckets.  Which of the two is
# the representative (S1, ordered by the count kernel) and which goes to S2 (ordered by the merge) is decided by the 31-mer's middle
# base, the first of the 8 (kmer_bits.h rep_orientation: A or C keeps the k-mer, G or T takes its reverse complement): so one case
# puts the one bucket of 5 000 into the count kernel and one into the merge
digest("one_bucket", as_rows(crowded(5, 5000, "C" * 7, "AC")), 31)
digest("one_bucket_in_merge", as_rows(crowded(6, 5000, "C" * 7, "GT")), 31)
# every second read twice and weights below 2 dropped: kept and dropped entries side by side in the table
reads = crowded(9000, 9000)
digest("kept_and_dropped", as_rows(reads + reads[::2]), 31, 2)
# the same with more kept keys than leave the table's tail free: 18 500 in the table, 17 800 of them kept
reads = crowded(18500, 18500)
digest("past_the_tail_kept", as_rows(reads + reads[:17800]), 31, 2)
# remainders of 6 and 10 bits: fewer than the bucket bits
for k in (11, 13):
    digest("k%d" % k, o.synth_reads(k, 4000, 150, 30000, 3e-3, 0), k)
"""

# the ring-wrap case against the oracle's sequential build, as tests/test_gpu_build.py compares: counts, the ascending k-mers, the
# (label, weight) multiset, and the node ids of every edge's two ends
_ORACLE_SCRIPT = _COMMON + r"""
from katome_amd.build import GpuGraph
k = 31
reads = as_rows(crowded(9000, 9000))
g, rb = GpuGraph.create_from_packed(pack_reads_ascii(reads).reshape(-1), len(reads), reads.shape[1], reverse_complement=True, k=k)
ref = o.build_ascii(reads, k, True)
assert rb == ref.read_bytes == reads.size
assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges), (g.n_nodes, g.n_edges, ref.n_nodes, ref.n_edges)
ek = g.key_ints("edge")
assert ek == sorted(kmer_to_int(s) for s in ref.kmer_strings())
assert g.multiset() == ref.multiset()
nk = g.key_ints("node")
assert len(set(nk)) == len(nk) == g.n_nodes
mask = (1 << (2 * (k - 1))) - 1
src, dst = g.edge_src.tolist(), g.edge_dst.tolist()
for e in range(g.n_edges):
    assert nk[src[e]] == ek[e] >> 2 and nk[dst[e]] == ek[e] & mask, e
print("ORACLE_OK", g.n_nodes, g.n_edges, flush=True)
"""

_GROUPED = "ordered per group in the merge"
_FULL = "too large for the merge's LDS; sorted in full"
_ROUTES = {"default": {}, "s2_sort": {"KATOME_S2_GROUP_SORT": "0"}, "edge_sort": {"KATOME_EDGE_HALF_SORT": "0"}, "capped": {"KATOME_S2_GROUP_CAP": "1"}}
_CASES = ["one_step", "several_steps", "ring_wrap", "large_group", "over_the_cap", "past_the_tail", "one_bucket", "one_bucket_in_merge",
          "kept_and_dropped", "past_the_tail_kept", "k11", "k13"]
_COUNTED_IN_ORDER = "[lds count] in key order, 8-byte slots, 1 visit(s) per record: code 0"
_GAVE_UP = "counting by hash groups"


def _env(**extra):
    # (KATOME_SORTED_COUNT=2: the k-mer level counted by sorting however small the input)
    return dict(os.environ, KATOME_SORTED_COUNT="2", KATOME_LC_TRACE="1", **extra)


@pytest.fixture(scope="module")
def routes():
    """route -> (case -> its LO row, case -> the trace lines of its build); the four processes run side by side"""
    procs = {name: subprocess.Popen([sys.executable, "-c", _DIGEST_SCRIPT, ROOT], env=_env(**extra), stdout=subprocess.PIPE,
                                    stderr=subprocess.PIPE, text=True) for name, extra in _ROUTES.items()}
    res = {}
    try:
        for name, p in procs.items():
            out, err = p.communicate(timeout=600)
            assert p.returncode == 0, (name, err[-3000:])
            rows = {line.split()[1]: line for line in out.splitlines() if line.startswith("LO ")}
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


def _s2_line(trace_lines):
    """(largest S2 group, the rest of the line) of a build's "[half sort] S2" trace line, or None"""
    for line in trace_lines:
        m = re.search(r"\[half sort\] S2: (\d+) keys, largest group (\d+): (.*)", line)
        if m:
            return int(m.group(2)), m.group(3)
    return None


@pytest.mark.parametrize("case", _CASES)
def test_every_route_gives_the_same_arrays(routes, case):
    rows = routes["default"][0]
    assert case in rows
    for name in _ROUTES:
        assert routes[name][0].get(case) == rows[case], (name, case)


@pytest.mark.parametrize("case,n", [("one_step", 1000), ("several_steps", 3000), ("ring_wrap", 9000), ("large_group", 14000),
                                    ("one_bucket", 5000), ("one_bucket_in_merge", 5000), ("kept_and_dropped", 4500)])
def test_the_crowded_group_is_ordered_in_the_merge(routes, case, n):
    """group 0 reached the size the case means, in the count's table and in the merge's LDS, and no way back was taken"""
    trace = routes["default"][1]
    s2 = _s2_line(trace[case])
    assert s2 is not None, trace[case]
    assert s2[0] == n and _GROUPED in s2[1], s2
    assert any(_COUNTED_IN_ORDER in line for line in trace[case]) and not any(_GAVE_UP in line for line in trace[case]), trace[case]
    # the routes that are compared against did take their own ways
    assert _s2_line(routes["s2_sort"][1][case]) is None and _s2_line(routes["edge_sort"][1][case]) is None
    capped = _s2_line(routes["capped"][1][case])
    assert capped is not None and _FULL in capped[1], capped


@pytest.mark.parametrize("case,n", [("over_the_cap", 17000), ("past_the_tail", 18000), ("past_the_tail_kept", 17800)])
def test_a_group_over_the_cap_is_counted_in_order_and_sorted_in_full(routes, case, n):
    """more keys in one group than the merge's LDS holds (16 368): the ordered count still completes at that size and S2 is sorted in
    full.  17 000 kept keys leave the count table's tail to the 8192 buckets; 18 000, and 17 800 kept of 18 500, are more than the
    17 406 that do, so the count kernel orders them in the 2048 buckets behind the table.  The arrays are those of the other routes
    (above)"""
    trace = routes["default"][1]
    s2 = _s2_line(trace[case])
    assert s2 is not None, trace[case]
    assert s2[0] == n and _FULL in s2[1], s2
    assert any(_COUNTED_IN_ORDER in line for line in trace[case]) and not any(_GAVE_UP in line for line in trace[case]), trace[case]


def test_few_remainder_bits_take_the_grouped_merge(routes):
    for case in ("k11", "k13"):
        s2 = _s2_line(routes["default"][1][case])
        assert s2 is not None and _GROUPED in s2[1], routes["default"][1][case]


def test_a_crowded_group_equals_the_oracle():
    out = subprocess.run([sys.executable, "-c", _ORACLE_SCRIPT, ROOT], env=_env(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ORACLE_OK" in out.stdout
    s2 = _s2_line(out.stderr.splitlines())
    assert s2 is not None and s2[0] == 9000 and _GROUPED in s2[1], out.stderr[-2000:]
