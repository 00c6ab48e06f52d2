"""Times the path region of the assembly's BIDIRECTED GFA (katome_dev_collapse_gfa_strands, katome_dev_gfa_strand_paths_arrays) beside a
plain copy of the same bytes, beside the two-strand writer (gfa_paths_write_kernel) in the same run, and the parts of the mirror search:
python tools/bench_gfa_strand_paths.py [--reads 2000000] [--pieces 50000000] [--runs 3]   -> one JSON line

The two inputs of tools/bench_gfa_paths.py:
  * an assembly: a by-key build of C3's first --reads reads (150 bp, k = 31, both strands), collapse() once (not timed), then every run
    times katome_dev_collapse_gfa and katome_dev_collapse_gfa_strands, alternated, from the phase table (HIP events around the
    launches): "k:gfa_paths_write_kernel" and "k:gfa_strand_paths_write_kernel" on their P lines, each beside hipMemcpyAsync device to
    device of as many bytes, and the mirror search's "k:mirror_sig_kernel", "k:mirror signature sort", "k:mirror_search_kernel" and
    "k:mirror_verify_kernel" (verify and settle, every round);
  * the synthetic walk of --pieces pieces round a cycle of 2^20 edges, a contig every 50 pieces and a jump every 100 on average,
    through katome_dev_gfa_paths_arrays and katome_dev_gfa_strand_paths_arrays (KATOME_GFA_PATHS_TRACE=1 and
    KATOME_GFA_STRAND_PATHS_TRACE=1 print the kernels' times), with twin(i) = i ^ 1: half the pieces read '-', and the one-piece paths
    find mirrors among themselves.
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
os.environ["KATOME_GFA_STRAND_PATHS_TRACE"] = "1"
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
MIRROR = {"k:mirror_sig_kernel": "mirror_sig_ms", "k:mirror signature sort": "mirror_sort_ms", "k:mirror_search_kernel": "mirror_search_ms",
          "k:mirror_verify_kernel": "mirror_verify_ms"}


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


def finish(d, runs, two_bytes, merged_bytes):
    for n, v in runs.items():
        d[n] = summary(v)
    d["paths_write_GBps"] = gbps(two_bytes, d["paths_write_ms"]["median"])
    d["paths_write_rate_over_copy"] = d["paths_copy_ms"]["median"] / d["paths_write_ms"]["median"]
    d["strand_paths_write_GBps"] = gbps(merged_bytes, d["strand_paths_write_ms"]["median"])
    d["strand_paths_write_rate_over_copy"] = d["strand_paths_copy_ms"]["median"] / d["strand_paths_write_ms"]["median"]
    d["mirror_ms"] = sum(d[n]["median"] for n in MIRROR.values())


out = {}
names = ["paths_write_ms", "paths_copy_ms", "strand_paths_write_ms", "strand_paths_copy_ms"] + list(MIRROR.values()) + ["mirror_rounds"]

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
out.update(contigs=a.n_contigs, pieces=a.n_pieces, simple_loops=a.stats["simple_loops"])
del a
b.profile(True)
runs = {n: [] for n in names}
for run in range(args.runs + 1):                # (run 0: warm-up)
    torch.cuda.synchronize()
    b.profile_read()
    g = b.collapse_gfa()
    prof = b.profile_read()
    vals = [prof["k:gfa_paths_write_kernel"][0], copy_ms(g.path_text, g.path_bytes)]
    out.update(paths=g.n_paths, jumps=g.n_jumps, path_bytes=g.path_bytes)
    del g
    g = b.collapse_gfa(merge_strands=True)
    prof = b.profile_read()
    vals += [prof["k:gfa_strand_paths_write_kernel"][0], copy_ms(g.path_text, g.path_bytes)]
    vals += [prof[k][0] if k in prof else 0.0 for k in MIRROR] + [prof["k:mirror_verify_kernel"][1] if "k:mirror_verify_kernel" in prof else 0]
    assert (g.n_paths, g.n_jumps) == (out["paths"], out["jumps"])
    out.update(segments=g.n_segments, links=g.n_links, unpaired=g.n_unpaired, self_twins=g.n_self_twins, strand_path_bytes=g.path_bytes, mirrored=g.n_mirrored,
               self_mirror=g.n_self_mirror)
    del g
    if run:
        for n, v in zip(names, vals):
            runs[n].append(v)
finish(out, runs, out["path_bytes"], out["strand_path_bytes"])
b.close()

# ---- a synthetic walk ----------------------------------------------------------------------------------------------------------
n_edges, P = 1 << 20, args.pieces
gen = torch.Generator(device="cuda").manual_seed(1)
src = torch.arange(n_edges, dtype=torch.int64, device="cuda")
dst = (src + 1) % n_edges
twin = src ^ 1
ids = torch.arange(P, dtype=torch.int64, device="cuda") % n_edges
u = torch.rand(P, device="cuda", generator=gen)
ids = torch.where(u < 0.01, torch.randint(0, n_edges, (P,), device="cuda", generator=gen), ids)      # a jump in, and most often one out
whole = (u > 0.98)
whole[0] = True
pieces = (ids | (whole.to(torch.int64) << 31)).to(torch.int32)      # (bit 31 set: the int32 wraps to the u32 the library reads)
del ids, u, whole
runs = {n: [] for n in names}
syn = {}
for run in range(args.runs + 1):
    (text, counts, line_off, contig, first), err = traced(lambda: kd.gfa_paths_arrays(src, dst, pieces))
    m = re.search(r"k:gfa_paths_write_kernel ([0-9.]+) ms, (\d+) bytes, (\d+) pieces, (\d+) paths", err)
    assert m and int(m.group(2)) == counts["text_bytes"] and int(m.group(3)) == P, err
    vals = [float(m.group(1)), copy_ms(text, counts["text_bytes"])]
    syn.update(pieces=P, edges=n_edges, paths=counts["n_paths"], jumps=counts["n_jumps"], path_bytes=counts["text_bytes"])
    del text, line_off, contig, first
    (text, counts, line_off, contig, first, mirror), err = traced(lambda: kd.gfa_strand_paths_arrays(src, dst, twin, pieces))
    got = {}
    for name, ms in re.findall(r"\[katome_dev_gfa_strand_paths_arrays\] (k:[^0-9]*?) ([0-9.]+) ms", err):
        got.setdefault(name, []).append(float(ms))
    assert "k:gfa_strand_paths_write_kernel" in got and (counts["n_paths"], counts["n_jumps"]) == (syn["paths"], syn["jumps"]), err
    vals += [sum(got["k:gfa_strand_paths_write_kernel"]), copy_ms(text, counts["text_bytes"])]
    vals += [sum(got.get(k, [0.0])) for k in MIRROR] + [len(got.get("k:mirror_verify_kernel", []))]
    syn.update(strand_path_bytes=counts["text_bytes"], mirrored=counts["n_mirrored"], self_mirror=counts["n_self_mirror"])
    del text, line_off, contig, first, mirror
    if run:
        for n, v in zip(names, vals):
            runs[n].append(v)
finish(syn, runs, syn["path_bytes"], syn["strand_path_bytes"])
out["synthetic"] = syn
print(json.dumps(out), flush=True)
