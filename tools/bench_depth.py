"""Times katome_dev_depth against a route made only of entries that were there before it:
    python tools/bench_depth.py [--reads 20000000] [--batch-reads 4000000] [--runs 3]
-> one JSON line

The graph is a by-key build of C3's first --reads reads (150 bp, k = 31, both strands).  The same reads are then queried in batches
(a call takes fewer than 2^32 windows):
  * fused:     Builder.depth, summary only -- one kernel, no record array, no rank array;
  * yardstick: katome_dev_extract_var on a scratch builder with reverse_complement = 0 (every window's key as spelled),
               rank_in_sorted against the graph's keys, a gather of the weights and their sum;
  * fused with WINDOWS, fused with EDGE_HITS.
The fused summary and the yardstick alternate --runs times after one warm-up each; per quantity the median and (min, max) of the
windows per second over the runs.  Also: the index build's time ("k:depth_index" of the profile, first call), the bytes the index
holds, and the kernel's own time per batch ("k:depth_kernel")."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=20_000_000)
ap.add_argument("--batch-reads", type=int, default=4_000_000)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

import torch  # noqa: E402
from katome_amd import device as kd  # noqa: E402
from katome_amd.workloads import WORKLOADS  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


w = WORKLOADS["c3"].scaled(args.reads)
k, L = w.k, w.read_len
packed, skip = kd.synth_reads(0, w.reads, L, w.genome_len, w.err_rate, 0, device=0)
b = kd.Builder(k, True, table_slots_hint=int(w.expected_distinct_canonical() * 2.2))
for r0 in range(0, w.reads, 4 << 20):
    b.count_reads(packed, min(4 << 20, w.reads - r0), L, None, first_read=r0)
dg = b.finalize()
stride, W = (L + 3) // 4, L - k + 1
batches = [(r0, min(args.batch_reads, w.reads - r0)) for r0 in range(0, w.reads, args.batch_reads)]
n_max = max(n for _, n in batches)
off = torch.arange(n_max + 1, dtype=torch.int64, device="cuda") * stride
lens = torch.full((n_max,), L, dtype=torch.int32, device="cuda")
prefix = torch.arange(n_max + 1, dtype=torch.int64, device="cuda") * W
scratch = kd.Builder(k, False)
records = torch.empty(n_max * W, dtype=torch.int64, device="cuda")
windows = w.reads * W


def fused(**flags):
    total = 0
    for r0, n in batches:
        r = b.depth(packed[r0 * stride:(r0 + n) * stride], off[:n], lens[:n], "packed", **flags)
        total += r.weight_sum
        assert r.n_windows == n * W
        del r
    return total


def yardstick():
    total = 0
    for r0, n in batches:
        rec = scratch.extract_var(packed[r0 * stride:(r0 + n) * stride], off[:n + 1], lens[:n], prefix[:n + 1], n * W, out=records)
        rank = kd.rank_in_sorted(dg.edge_key, rec, 2 * k, 1)
        found = rank >= 0
        total += int(dg.edge_weight[rank.clamp(min=0)].to(torch.int64).mul(found).sum().item())
        del rank, found
    return total


out = {"reads": w.reads, "k": k, "edges": dg.n_edges, "windows": windows, "batches": len(batches)}
b.profile(True)
b.profile_read()
want, first = timed(fused)                          # (warm-up; builds the index)
prof = b.profile_read()
out["index_build_ms"] = prof["k:depth_index"][0]
out["index_bytes"] = b.depth_index_bytes()
out["first_call_s"] = first
assert yardstick() == want                          # (warm-up; and the two routes agree)
runs = {"fused": [], "yardstick": [], "kernel_ms": []}
for _ in range(args.runs):
    b.profile_read()
    got, s = timed(fused)
    assert got == want
    runs["kernel_ms"].append(b.profile_read()["k:depth_kernel"][0])
    runs["fused"].append(windows / s)
    got, s = timed(yardstick)
    assert got == want
    runs["yardstick"].append(windows / s)
for name, flags in (("fused_windows", dict(windows=True)), ("fused_edge_hits", dict(edge_hits=True)), ("fused_either_strand", dict(either_strand=True))):
    fused(**flags)
    xs = []
    for _ in range(args.runs):
        got, s = timed(lambda: fused(**flags))
        assert got == want
        xs.append(windows / s)
    out[name + "_windows_per_s"] = spread(xs)
out["fused_windows_per_s"], out["yardstick_windows_per_s"] = spread(runs["fused"]), spread(runs["yardstick"])
out["depth_kernel_ms_per_pass"] = spread(runs["kernel_ms"])
# the bar, strictly: the slowest fused run is not below the fastest yardstick run
out["fused_not_slower"] = out["fused_windows_per_s"]["min"] >= out["yardstick_windows_per_s"]["max"]
out["footprint_bytes"] = dg.n_edges * (8 + 4) + out["index_bytes"]          # keys, weights and the directory: what a lookup reads from
print(json.dumps(out), flush=True)
