"""Times the path region of the assembly's GFA (katome_dev_collapse_gfa, katome_dev_gfa_paths_arrays) beside a plain copy of the same
bytes and beside the unitig writer's own ratio in the same run:
python tools/bench_gfa_paths.py [--reads 2000000] [--pieces 50000000] [--runs 3]   -> one JSON line

Two inputs:
  * an assembly: a by-key build of C3's first --reads reads (150 bp, k = 31, both strands), collapse() once (its exact shrink and
    its walk are one host core's and are not timed here), then every run times katome_dev_collapse_gfa from the phase table (HIP
    events around the launches): "k:gfa_write_kernel" on the H / S / L part and "k:gfa_paths_write_kernel" on the P lines, each beside
    hipMemcpyAsync device to device of as many bytes as that part has, HIP events on the same stream;
  * a synthetic walk of --pieces pieces round a cycle of 2^20 edges, a contig every 50 pieces and a jump every 100 on average,
    through katome_dev_gfa_paths_arrays (KATOME_GFA_PATHS_TRACE=1 prints the writer's time): a path region large enough to time,
    which an assembly's is not (its pieces are the shrunk edges' weights added up).
What it prints: per quantity the median and the spread (min, max) over the runs; each writer's GB/s of text written and its rate over
the copy's."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["KATOME_GFA_PATHS_TRACE"] = "1"
import torch  # noqa: E402

from katome_amd import device as kd  # noqa: E402
from katome_amd.workloads import WORKLOADS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--pieces", type=int, default=50_000_000)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]


def copy_ms(src, n):
    dst = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda")
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


med = statistics.median
gbps = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9
summary = lambda v: {"median": med(v), "min": min(v), "max": max(v)}
out = {}

# ---- an assembly ---------------------------------------------------------------------------------------------------------------
w = WORKLOADS["c3"].scaled(args.reads)
packed, skip = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, 0, device=0)
b = kd.Builder(w.k, True, table_slots_hint=int(w.expected_distinct_canonical() * 2.2))
step = 4 << 20
for r0 in range(0, w.reads, step):
    b.count_reads(packed, min(step, w.reads - r0), w.read_len, None, first_read=r0)
dg = b.finalize()
out.update(reads=w.reads, k=w.k, genome_len=w.genome_len, edges=dg.n_edges, nodes=dg.n_nodes)
del dg, packed, skip
a = b.collapse("fasta")
out.update(contigs=a.n_contigs, pieces=a.n_pieces, simple_loops=a.stats["simple_loops"], collapse_host_ms=a.stats["host_ms"],
           shrink_host_ms=a.stats["shrink_host_ms"])
del a
b.profile(True)
names = ["gfa_write_ms", "gfa_copy_ms", "paths_write_ms", "paths_copy_ms"]
runs = {n: [] for n in names}
for run in range(args.runs + 1):                # (run 0: warm-up)
    torch.cuda.synchronize()
    b.profile_read()
    g = b.collapse_gfa()
    prof = b.profile_read()
    vals = [prof["k:gfa_write_kernel"][0], copy_ms(g.text, g.text_bytes), prof["k:gfa_paths_write_kernel"][0], copy_ms(g.path_text, g.path_bytes)]
    out.update(segments=g.n_segments, links=g.n_links, gfa_bytes=g.text_bytes, paths=g.n_paths, jumps=g.n_jumps, path_bytes=g.path_bytes)
    del g
    if run:
        for n, v in zip(names, vals):
            runs[n].append(v)
for n in names:
    out[n] = summary(runs[n])
out["gfa_write_GBps"] = gbps(out["gfa_bytes"], out["gfa_write_ms"]["median"])
out["gfa_write_rate_over_copy"] = out["gfa_copy_ms"]["median"] / out["gfa_write_ms"]["median"]
out["paths_write_GBps"] = gbps(out["path_bytes"], out["paths_write_ms"]["median"])
out["paths_write_rate_over_copy"] = out["paths_copy_ms"]["median"] / out["paths_write_ms"]["median"]
b.close()

# ---- a synthetic walk ----------------------------------------------------------------------------------------------------------
n_edges, P = 1 << 20, args.pieces
gen = torch.Generator(device="cuda").manual_seed(1)
src = torch.arange(n_edges, dtype=torch.int64, device="cuda")
dst = (src + 1) % n_edges
ids = torch.arange(P, dtype=torch.int64, device="cuda") % n_edges
u = torch.rand(P, device="cuda", generator=gen)
ids = torch.where(u < 0.01, torch.randint(0, n_edges, (P,), device="cuda", generator=gen), ids)      # a jump in, and most often one out
whole = (u > 0.98)
whole[0] = True
pieces = (ids | (whole.to(torch.int64) << 31)).to(torch.int32)      # (bit 31 set: the int32 wraps to the u32 the library reads)
del ids, u, whole
syn = {n: [] for n in ("write_ms", "copy_ms")}
for run in range(args.runs + 1):
    (text, counts, line_off, contig, first), err = traced(lambda: kd.gfa_paths_arrays(src, dst, pieces))
    m = re.search(r"k:gfa_paths_write_kernel ([0-9.]+) ms, (\d+) bytes, (\d+) pieces, (\d+) paths", err)
    assert m and int(m.group(2)) == counts["text_bytes"] and int(m.group(3)) == P, err
    cp = copy_ms(text, counts["text_bytes"])
    del text, line_off, contig, first
    if run:
        syn["write_ms"].append(float(m.group(1)))
        syn["copy_ms"].append(cp)
out["synthetic"] = dict(pieces=P, edges=n_edges, paths=counts["n_paths"], jumps=counts["n_jumps"], path_bytes=counts["text_bytes"],
                        paths_write_ms=summary(syn["write_ms"]), paths_copy_ms=summary(syn["copy_ms"]),
                        paths_write_GBps=gbps(counts["text_bytes"], med(syn["write_ms"])),
                        paths_write_rate_over_copy=med(syn["copy_ms"]) / med(syn["write_ms"]))
print(json.dumps(out), flush=True)
