"""Times the bidirected GFA export of a shrunk graph (katome_dev_contigs_gfa_strands: strand twins merged) beside the two-strand
export (katome_dev_contigs_gfa) of the same shrink result:
python tools/bench_gfa_strands.py [--reads 20000000] [--runs 3]   -> one JSON line

The input is that of tools/bench_gfa.py: a by-key build of C3's first --reads reads (150 bp, k = 31, both strands) and the
traversal-free shrink.  Every run times, one after the other (so that the two alternate --runs times):
  * katome_dev_contigs_gfa: the call's wall time and its kernels from the phase table ("k:gfa link sort", "k:gfa sizes",
    "k:gfa_write_kernel");
  * katome_dev_contigs_gfa_strands: the call's wall time and its parts from the phase table -- the join it takes from gfa.hip
    ("k:gfa link sort" + "k:gfa sizes" again), "k:gfa_strands keys+sort" (the end k-mers, the sort of the first k-mers, the check for equal
    neighbours), "k:strand_search_kernel" (the bucket index over the sorted keys and the search), "k:strand_verify_kernel" (the pairs, the scan of their words and the comparison),
    "k:gfa_strands links" (the canonical keys, their sort and dev_unique), "k:gfa_strands sizes" and "k:gfa_strands_write_kernel".
    The parts that bring a count back to the host hold that wait too: they are HIP events around the launches.
What it prints: per quantity the median and the spread (min, max) over the runs; both writers' GB/s of text written; the
comparison's GB/s over the labels' bytes (what it must read, once); segment and link counts, file sizes and their ratio,
n_unpaired and n_self_twins."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from katome_amd import device as kd  # noqa: E402
from katome_amd.workloads import WORKLOADS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=20_000_000)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

w = WORKLOADS["c3"].scaled(args.reads)
packed, skip = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, 0, device=0)
b = kd.Builder(w.k, True, table_slots_hint=int(w.expected_distinct_canonical() * 2.2))
step = 4 << 20
for r0 in range(0, w.reads, step):
    b.count_reads(packed, min(step, w.reads - r0), w.read_len, None, first_read=r0)
dg = b.finalize()
out = {"reads": w.reads, "k": w.k, "genome_len": w.genome_len, "edges": dg.n_edges, "nodes": dg.n_nodes}
del dg, packed, skip
dc = b.shrink("fast")
out.update(merged_edges=dc.n_edges, vertices=dc.n_nodes, label_bytes=dc.label_bytes)

TWO = {"two_strand_sort_ms": "k:gfa link sort", "two_strand_sizes_ms": "k:gfa sizes", "two_strand_write_ms": "k:gfa_write_kernel"}
MERGED = {"join_sort_ms": "k:gfa link sort", "join_sizes_ms": "k:gfa sizes", "keys_ms": "k:gfa_strands keys+sort", "search_ms": "k:strand_search_kernel", "verify_ms": "k:strand_verify_kernel",
          "links_ms": "k:gfa_strands links", "sizes_ms": "k:gfa_strands sizes", "write_ms": "k:gfa_strands_write_kernel"}
names = ["two_strand_wall_ms", "merged_wall_ms"] + list(TWO) + list(MERGED)
runs = {n: [] for n in names}
b.profile(True)
for run in range(args.runs + 1):                # (run 0: warm-up)
    torch.cuda.synchronize()
    b.profile_read()
    t0 = time.perf_counter()
    g = dc.gfa()
    torch.cuda.synchronize()
    wall_two = (time.perf_counter() - t0) * 1e3
    prof_two = b.profile_read()
    two = (g.n_segments, g.n_links, g.text_bytes)
    del g
    t0 = time.perf_counter()
    g = dc.gfa(merge_strands=True)
    torch.cuda.synchronize()
    wall_merged = (time.perf_counter() - t0) * 1e3
    prof = b.profile_read()
    merged = (g.n_segments, g.n_links, g.text_bytes, g.n_unpaired, g.n_self_twins)
    del g
    if run:
        runs["two_strand_wall_ms"].append(wall_two)
        runs["merged_wall_ms"].append(wall_merged)
        for n, ph in TWO.items():
            runs[n].append(prof_two[ph][0])
        for n, ph in MERGED.items():
            runs[n].append(prof[ph][0] if ph in prof else 0.0)

for n in names:
    out[n] = {"median": statistics.median(runs[n]), "min": min(runs[n]), "max": max(runs[n])}
gbps = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9 if ms > 0 else None
out.update(two_strand_segments=two[0], two_strand_links=two[1], two_strand_bytes=two[2], segments=merged[0], links=merged[1], bytes=merged[2],
           n_unpaired=merged[3], n_self_twins=merged[4], bytes_ratio=merged[2] / two[2])
out["two_strand_write_GBps"] = gbps(two[2], out["two_strand_write_ms"]["median"])
out["write_GBps"] = gbps(merged[2], out["write_ms"]["median"])
out["verify_GBps_of_label_bytes"] = gbps(dc.label_bytes, out["verify_ms"]["median"])
out["two_strand_kernels_ms"] = sum(out[n]["median"] for n in TWO)
out["merged_kernels_ms"] = sum(out[n]["median"] for n in MERGED)
out["merged_over_two_strand_wall"] = out["merged_wall_ms"]["median"] / out["two_strand_wall_ms"]["median"]
del dc
b.close()
print(json.dumps(out), flush=True)
