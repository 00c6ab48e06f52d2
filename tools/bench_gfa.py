"""Times the GFA export of a shrunk graph (katome_dev_contigs_gfa) beside the unitig FASTA of the same shrink result and a plain copy:
python tools/bench_gfa.py [--reads 20000000] [--runs 3]   -> one JSON line

The input is a by-key build of C3's first --reads reads (150 bp, k = 31, both strands) and the traversal-free shrink.  Every run
times, one after the other (so that the three alternate --runs times):
  * katome_dev_contigs_gfa with its kernels, from the phase table (HIP events around the launches): "k:gfa link sort" (dev_sort of
    the edge indices by source), "k:gfa sizes" (the checks, the vertex ranges, the link counts, the two scans, the links' fill) and
    "k:gfa_write_kernel"; the call's wall time beside them;
  * katome_dev_contigs_text in FASTA layout on the same shrink result ("k:text_write_kernel");
  * hipMemcpyAsync device to device of as many bytes as the GFA has, HIP events on the same stream;
  * the S region alone: katome_dev_gfa_arrays (KATOME_GFA_TRACE=1 prints the writer's time) on the same arrays with every edge_dst
    pointed at one extra vertex without out-edges, which leaves the header and the S lines and no link.
What it prints: per quantity the median and the spread (min, max) over the runs; the writer's GB/s of text written; its rate over the
FASTA writer's and over the copy's; the S region's rate over the FASTA writer's on the same bases; the L region's share of the file
and its rate, derived as (L bytes) / (whole writer - S-only writer)."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["KATOME_GFA_TRACE"] = "1"
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
out.update(segments=dc.n_edges, vertices=dc.n_nodes, label_bytes=dc.label_bytes)

hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]


def copy_ms(src, dst, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n, 3, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    e1.record()
    torch.cuda.synchronize()
    assert rc == 0
    return e0.elapsed_time(e1)


def traced(fn):
    """fn() with the library's stderr caught -> (fn's result, what it wrote)"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return res, f.read().decode()


sink_dst = torch.full_like(dc.edge_dst, dc.n_nodes)       # every edge ends in one extra vertex that has no out-edges: no links


def s_region_only():
    g, err = traced(lambda: kd.gfa_arrays(w.k, dc.n_nodes + 1, dc.edge_src, sink_dst, dc.edge_weight, dc.edge_kmers, dc.edge_label_off, dc.edge_label,
                                          label_bytes=dc.label_bytes))
    m = re.search(r"k:gfa_write_kernel ([0-9.]+) ms, (\d+) bytes, \d+ segments, (\d+) links", err)
    assert m and int(m.group(3)) == 0 and g.n_links == 0, err
    return float(m.group(1)), int(m.group(2))


b.profile(True)
names = ["gfa_wall_ms", "gfa_sort_ms", "gfa_sizes_ms", "gfa_write_ms", "fasta_write_ms", "copy_ms", "s_only_write_ms"]
runs = {n: [] for n in names}
for run in range(args.runs + 1):                # (run 0: warm-up)
    torch.cuda.synchronize()
    b.profile_read()
    t0 = time.perf_counter()
    g = dc.gfa()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    prof = b.profile_read()
    gfa_bytes, n_links = g.text_bytes, g.n_links
    dst = torch.empty(gfa_bytes, dtype=torch.uint8, device="cuda")
    fa = dc.text("fasta")
    prof_fa = b.profile_read()
    fasta_bytes = fa.text_bytes
    cp = copy_ms(g.text, dst, gfa_bytes)
    del g, fa, dst
    s_ms, s_bytes = s_region_only()
    if run:
        for n, v in zip(names, [wall, prof["k:gfa link sort"][0], prof["k:gfa sizes"][0], prof["k:gfa_write_kernel"][0],
                                prof_fa["k:text_write_kernel"][0], cp, s_ms]):
            runs[n].append(v)

med = statistics.median
for n in names:
    out[n] = {"median": med(runs[n]), "min": min(runs[n]), "max": max(runs[n])}
gbps = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9
l_bytes = gfa_bytes - s_bytes                   # (the S-only text is the header and the S lines, byte for byte those of the whole text)
bases = int(dc.edge_kmers.to(torch.int64).sum().item()) + dc.n_edges * (w.k - 1)      # the same in both texts
out.update(gfa_bytes=gfa_bytes, links=n_links, fasta_bytes=fasta_bytes, s_region_bytes=s_bytes, l_region_bytes=l_bytes,
           l_region_share=l_bytes / gfa_bytes, bases=bases)
out["gfa_write_GBps"] = gbps(gfa_bytes, out["gfa_write_ms"]["median"])
out["fasta_write_GBps"] = gbps(fasta_bytes, out["fasta_write_ms"]["median"])
out["copy_GBps"] = gbps(gfa_bytes, out["copy_ms"]["median"])
out["gfa_write_rate_over_fasta"] = out["gfa_write_GBps"] / out["fasta_write_GBps"]
out["gfa_write_rate_over_copy"] = out["gfa_write_GBps"] / out["copy_GBps"]
out["s_only_write_GBps"] = gbps(s_bytes, out["s_only_write_ms"]["median"])
# the same bases through both writers: bases per second, S region over FASTA (and the FASTA writer's spread, to read it against)
out["s_region_bases_rate_over_fasta"] = out["fasta_write_ms"]["median"] / out["s_only_write_ms"]["median"]
out["fasta_write_spread"] = (out["fasta_write_ms"]["max"] - out["fasta_write_ms"]["min"]) / out["fasta_write_ms"]["median"]
l_ms = out["gfa_write_ms"]["median"] - out["s_only_write_ms"]["median"]
out["l_region_derived_ms"] = l_ms
out["l_region_derived_GBps"] = gbps(l_bytes, l_ms) if l_ms > 0 else None
del dc, sink_dst
b.close()
print(json.dumps(out), flush=True)
