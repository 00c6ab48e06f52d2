"""The reverse-complement half of the ordered k-mer count (S2) ordered group by group in LDS inside the merge (radix.hip
group_merge_kernel, KATOME_S2_GROUP_SORT) instead of sorted in full.  Every route must give byte for byte the arrays of the others:
the new one, the full S2 sort with half_merge_kernel (KATOME_S2_GROUP_SORT=0), the full edge sort (KATOME_EDGE_HALF_SORT=0) and the
way back when a group is larger than the merge takes (KATOME_S2_GROUP_CAP).  The switches are read once, so every route runs in a
process of its own."""
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
    print("GS", name, dg.n_nodes, dg.n_edges, h.hexdigest(), flush=True)
    b.close()

for k in (11, 13, 17, 21, 25, 31):                                    # odd k, both strands
    digest("k%d" % k, o.synth_reads(k, 4000, 150, 30000, 3e-3, 0), k, True)
digest("one_strand_k31", o.synth_reads(3, 3000, 150, 30000, 3e-3, 0), 31, False)
digest("min_weight", o.synth_reads(5, 4000, 150, 20000, 3e-3, 0), 31, True, 3)
digest("left_over_windows", o.synth_reads(6, 4000, 101, 30000, 3e-3, 0), 31, True)      # (101 bp: windows that are not whole tiles)
# low complexity: reads that begin with a run of A's -- their k-mers crowd a few 16-bit key prefixes
rng = random.Random(7)
lowc = ["A" * 37 + "".join(rng.choice("ACGT") for _ in range(23)) for _ in range(3000)]
digest("low_complexity", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 31, True)
rng = random.Random(8)
lowc = ["A" * 12 + "".join(rng.choice("ACGT") for _ in range(88)) for _ in range(3000)]
digest("low_complexity_short_run", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 21, True)
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

_GROUPED = "ordered per group in the merge"
_FULL = "too large for the merge's LDS; sorted in full"


def _run(script, args, timeout, **env_extra):
    env = dict(os.environ, KATOME_LC_TRACE="1", **env_extra)
    out = subprocess.run([sys.executable, "-c", script, ROOT] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def _rows(out, tag):
    return [line for line in out.stdout.splitlines() if line.startswith(tag + " ")]


def test_small_builds_equal_every_route():
    """odd k from 11 to 31, one strand, min_weight > 0, 101-bp reads and low-complexity input: the grouped merge, the full S2 sort,
    the full edge sort and the way back through the capacity hook give the same arrays"""
    # (KATOME_SORTED_COUNT=2: the k-mer level counted by sorting however small the input)
    new = _run(_SMALL_SCRIPT, [], 900, KATOME_SORTED_COUNT="2")
    s2_sort = _run(_SMALL_SCRIPT, [], 900, KATOME_SORTED_COUNT="2", KATOME_S2_GROUP_SORT="0")
    full = _run(_SMALL_SCRIPT, [], 900, KATOME_SORTED_COUNT="2", KATOME_EDGE_HALF_SORT="0")
    capped = _run(_SMALL_SCRIPT, [], 900, KATOME_SORTED_COUNT="2", KATOME_S2_GROUP_CAP="1")
    rows = _rows(new, "GS")
    assert len(rows) == 11
    assert _rows(s2_sort, "GS") == rows
    assert _rows(full, "GS") == rows
    assert _rows(capped, "GS") == rows
    # every two-strand build that is counted in order takes the grouped merge; one strand has no S2
    assert new.stderr.count(_GROUPED) >= 8, new.stderr[-2000:]
    assert _FULL not in new.stderr
    assert "[half sort] S2" not in s2_sort.stderr and "[half sort] S2" not in full.stderr
    assert capped.stderr.count(_FULL) >= 8 and _GROUPED not in capped.stderr, capped.stderr[-2000:]


def test_c2_equals_the_full_s2_sort():
    """C2 in full: weights, order and position-weighted checksums of every array as with the full S2 sort"""
    new = _run(_BIG_SCRIPT, ["c2"], 1200)
    old = _run(_BIG_SCRIPT, ["c2"], 1200, KATOME_S2_GROUP_SORT="0")
    assert _rows(new, "BIG")[-1] == _rows(old, "BIG")[-1]
    assert _GROUPED in new.stderr, new.stderr[-2000:]
