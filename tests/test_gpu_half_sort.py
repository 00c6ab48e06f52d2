"""The k-mer level counted in key order (lds_count.hip lds_count_ordered_kernel, KATOME_EDGE_HALF_SORT): the representatives leave the
count sorted, only their reverse complements are sorted, and one merge (radix.hip half_merge_kernel) makes the edge list.  The
arrays must be byte for byte those of the usual route (KATOME_EDGE_HALF_SORT=0), which sorts every edge.  The switch is read once,
so every route runs in a process of its own."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SMALL_SCRIPT = r"""
import sys, hashlib, random, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd

def digest(name, reads, k, rc, min_weight=0):
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
    print("HS", name, dg.n_nodes, dg.n_edges, h.hexdigest(), flush=True)
    b.close()

for k in (11, 15, 21, 25, 31):                                        # odd k, both strands
    digest("k%d" % k, o.synth_reads(k, 4000, 150, 30000, 3e-3, 0), k, True)
digest("one_strand_k31", o.synth_reads(3, 3000, 150, 30000, 3e-3, 0), 31, False)
digest("one_strand_k16", o.synth_reads(4, 3000, 100, 20000, 3e-3, 0), 16, False)
digest("min_weight", o.synth_reads(5, 4000, 150, 20000, 3e-3, 0), 31, True, 3)
digest("left_over_windows", o.synth_reads(6, 4000, 101, 30000, 3e-3, 0), 31, True)      # (101 bp: windows that are not whole tiles)
# low complexity: every window of a read begins with eight A's and the reads differ in their last 23 bases -- tens of thousands of
# distinct k-mers with one 16-bit key prefix, more than one group's table holds: the ordered count gives up and the level is
# counted by hash groups
rng = random.Random(7)
lowc = ["A" * 37 + "".join(rng.choice("ACGT") for _ in range(23)) for _ in range(3000)]
digest("low_complexity", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 31, True)
"""

_BIG_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from katome_amd import device as kd
from katome_amd.workloads import WORKLOADS
wl = WORKLOADS[sys.argv[2]]
packed, _ = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, 0)
b = kd.Builder(wl.k, True, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2))
for r0 in range(0, wl.reads, 4 << 20):
    b.count_reads(packed, min(4 << 20, wl.reads - r0), wl.read_len, None, first_read=r0)
del packed
dg = b.finalize()
sums = []
for a in (dg.edge_key.reshape(-1), dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key.reshape(-1), dg.edge_label.reshape(-1)):
    total, n = 0, a.numel()
    for i in range(0, n, 1 << 27):                     # sum of a[i] * (2 i + 1) mod 2^64: order and value of every word
        z = min(n, i + (1 << 27))
        w = torch.arange(i, z, device=a.device, dtype=torch.int64) * 2 + 1
        total = (total + int((a[i:z].to(torch.int64) * w).sum().item())) & ((1 << 64) - 1)
    sums.append(total)
print("BIG", dg.n_nodes, dg.n_edges, int(dg.edge_weight.to(torch.int64).sum().item()), *sums, flush=True)
"""


def _run(script, args, half, timeout, **extra):
    env = dict(os.environ, KATOME_EDGE_HALF_SORT=half, KATOME_LC_TRACE="1", **extra)
    out = subprocess.run([sys.executable, "-c", script, ROOT] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def test_small_builds_equal_the_sorted_route():
    """odd k from 11 to 31 on both strands, one strand (odd and even k), min_weight > 0, 101-bp reads and a low-complexity input
    that overflows a group's table (the fallback, under KATOME_LC_TRACE) -- every array byte for byte"""
    # (KATOME_SORTED_COUNT=2: the k-mer level counted by sorting however small the input)
    old = _run(_SMALL_SCRIPT, [], "0", 900, KATOME_SORTED_COUNT="2")
    new = _run(_SMALL_SCRIPT, [], "1", 900, KATOME_SORTED_COUNT="2")
    rows_old = [line for line in old.stdout.splitlines() if line.startswith("HS ")]
    rows_new = [line for line in new.stdout.splitlines() if line.startswith("HS ")]
    assert len(rows_old) == 10 and rows_new == rows_old
    assert "in key order" not in old.stderr
    assert new.stderr.count("in key order, 8-byte slots, 1 visit(s) per record: code 0") >= 8, new.stderr[-2000:]
    assert new.stderr.count("in key order: a group filled its table; counting by hash groups") == 1, new.stderr[-2000:]


@pytest.mark.parametrize("workload", ["c2", "c3"])
def test_full_workloads_equal_the_sorted_route(workload):
    """C2 and the benchmark's C3 in full: weights, order and position-weighted checksums of every array as the usual route's"""
    old = _run(_BIG_SCRIPT, [workload], "0", 1200)
    new = _run(_BIG_SCRIPT, [workload], "1", 1200)
    a = [line for line in old.stdout.splitlines() if line.startswith("BIG ")][-1]
    b = [line for line in new.stdout.splitlines() if line.startswith("BIG ")][-1]
    assert a == b, (a, b)
    assert "in key order, 8-byte slots, 1 visit(s) per record: code 0" in new.stderr, new.stderr[-2000:]
