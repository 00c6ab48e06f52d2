"""Times Collapsable::collapse on the device graph (katome_dev_collapse) for one synthetic input after the stages "dcwced":
python tools/bench_collapse.py [--reads 2000000] [--min-weight 2] [--reps 5] [--layout fasta]   -> one JSON line

What it prints: contigs, pieces and text bytes; host_ms of the walk (one host core, collapse_exact.h) and of the exact shrink in
front of it; the text kernel's time (HIP events around the launch: the "k:text_write_kernel" entry of the phase table) and its
GB/s of text written; and, timed with HIP events in the same run, a plain hipMemcpyAsync device-to-device of the same number of
bytes as the yardstick -- a copy reads and writes every byte once, the text kernel writes every byte once and reads a quarter of
it (2 bits per base) plus 12 bytes per piece.  Medians over --reps, after one warm-up.
The reads' contigs are short, so beside them ("long_*" in the output) the same kernel is timed through katome_dev_pieces_text on
hand-made input whose lanes take the 16-bases-per-store path: --long-pieces pieces (default 4096) over 64 random labels of
--long-bases bases (default 65536), one contig, plain layout; that call's time is a host clock around it (it measures, scans,
writes and synchronises), with the copy of as many bytes again as its yardstick."""
import argparse
import ctypes as C
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
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--min-weight", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layout", default="fasta", choices=["plain", "fasta"])
ap.add_argument("--long-pieces", type=int, default=4096)
ap.add_argument("--long-bases", type=int, default=65536)
args = ap.parse_args()

w = WORKLOADS["c3"].scaled(args.reads)
packed, skip = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, 0, device=0)
b = kd.Builder(w.k, True, table_slots_hint=int(w.expected_distinct_canonical() * 2.2), first_seen_order=True)
step = 4 << 20
for r0 in range(0, w.reads, step):
    b.count_reads(packed, min(step, w.reads - r0), w.read_len, None, first_read=r0)
dg = b.finalize()
out = {"reads": w.reads, "k": w.k, "genome_len": w.genome_len, "min_weight": args.min_weight, "layout": args.layout,
       "edges": dg.n_edges, "nodes": dg.n_nodes}
del dg, packed, skip
t0 = time.perf_counter()
b.remove_dead_paths()
b.standardize_contigs()
b.remove_weak_edges(args.min_weight)
b.standardize_contigs()
b.standardize_edges(w.genome_len, args.min_weight)
dg, _ = b.remove_dead_paths()
torch.cuda.synchronize()
out["stages_ms"] = (time.perf_counter() - t0) * 1e3
out["edges_after_stages"], out["nodes_after_stages"] = dg.n_edges, dg.n_nodes
del dg

b.profile(True)
kernel_ms, host_ms, shrink_host_ms, text_ms, wall_ms = [], [], [], [], []
for rep in range(args.reps + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a = b.collapse(args.layout)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    prof = b.profile_read()
    if rep:                                    # (rep 0: warm-up)
        wall_ms.append(wall)
        kernel_ms.append(prof["k:text_write_kernel"][0])
        host_ms.append(a.stats["host_ms"]); shrink_host_ms.append(a.stats["shrink_host_ms"]); text_ms.append(a.stats["text_ms"])
    st, text_bytes, n_contigs = a.stats, a.text_bytes, a.n_contigs
    del a
out.update(contigs=n_contigs, pieces=st["n_pieces"], text_bytes=text_bytes, shrunk_edges=st["shrunk_edges"], shrunk_nodes=st["shrunk_nodes"],
           steps=st["steps"], ambiguity_cuts=st["ambiguity_cuts"], self_loops=st["self_loops"], simple_loops=st["simple_loops"],
           scc_restarts=st["scc_restarts"], nodes_removed=st["nodes_removed"])
med = statistics.median
out.update(collapse_wall_ms=med(wall_ms), walk_host_ms=med(host_ms), shrink_host_ms=med(shrink_host_ms), text_total_ms=med(text_ms),
           text_kernel_ms=med(kernel_ms))
out["text_kernel_GBps"] = text_bytes / (out["text_kernel_ms"] * 1e-3) / 1e9 if text_bytes else 0.0

# the yardstick: hipMemcpyAsync device to device of n bytes, HIP events on the same stream
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]


def copy_ms(n):
    src = torch.full((n,), 65, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = []
    for rep in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n, 3, stream)      # hipMemcpyDeviceToDevice
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0
        if rep:
            ms.append(e0.elapsed_time(e1))
    return med(ms)


n = max(text_bytes, 16)
out["copy_d2d_ms"] = copy_ms(n)
out["copy_d2d_GBps"] = n / (out["copy_d2d_ms"] * 1e-3) / 1e9
out["text_kernel_fraction_of_copy_rate"] = out["text_kernel_GBps"] / out["copy_d2d_GBps"] if out["copy_d2d_GBps"] else 0.0

# long pieces through the primitive: 64 labels of --long-bases bases (whole bytes: pad 0), --long-pieces remainder pieces behind one whole one
if args.long_pieces:
    nb = args.long_bases // 4 * 4
    stride = 1 + nb // 4
    lab = torch.randint(0, 256, (64, stride), dtype=torch.uint8, device="cuda")
    lab[:, 0] = 0
    lab = torch.cat([lab.reshape(-1), torch.zeros(16, dtype=torch.uint8, device="cuda")])
    off = torch.arange(65, dtype=torch.int64, device="cuda") * stride
    gen = torch.Generator(device="cuda").manual_seed(1)
    pieces = torch.randint(0, 64, (args.long_pieces,), dtype=torch.int32, device="cuda", generator=gen)
    pieces[0] |= -(1 << 31)
    call_ms = []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, _, long_bytes = kd.pieces_text(lab, off, pieces, w.k, "plain")
        torch.cuda.synchronize()
        if rep:
            call_ms.append((time.perf_counter() - t0) * 1e3)
    # (the wrapper calls the entry twice -- a size query, then the write -- so a call measures and scans twice and writes once)
    out.update(long_pieces=args.long_pieces, long_bases=nb, long_text_bytes=long_bytes, long_call_ms=med(call_ms))
    out["long_call_GBps"] = long_bytes / (out["long_call_ms"] * 1e-3) / 1e9
    out["long_copy_d2d_ms"] = copy_ms(long_bytes)
    out["long_copy_d2d_GBps"] = long_bytes / (out["long_copy_d2d_ms"] * 1e-3) / 1e9
    out["long_call_fraction_of_copy_rate"] = out["long_call_GBps"] / out["long_copy_d2d_GBps"]
b.close()
print(json.dumps(out), flush=True)
