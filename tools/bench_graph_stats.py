"""CollectionStats and the weight spectrum on the device against the route they replace (copy the graph out, katome_graph_stats).
usage: python tools/bench_graph_stats.py [--reads 20000000] [--full] [--bins 4096] [--records-log2 28] [--reps 3]

A first-seen build of the first --reads reads of C3 (the size bench.py's next_stages uses), after remove_dead_paths; with
--full also C3 in full by packed key.  Every call is timed with a host clock around a call that ends in a synchronise, after
one warm-up, --reps repeats with the calls alternated; the kernels' own times come from the library's KATOME_STATS_TRACE lines
(HIP events around each launch), collected in a pass of their own because the trace waits for every kernel, and are priced against their algorithmic bytes as a share of the 8 TB/s HBM peak:
  stats_degree_kernel 32 B per edge (two 8-byte ids read, two 8-byte atomic adds), stats_weight_kernel and spectrum_kernel 4 B per
  record, stats_node_kernel 8 B per node.
The replaced route, in the same run: D2H of edge_src, edge_dst and edge_weight into host arrays, then katome_graph_stats.
The spectrum kernel alone, at 2^--records-log2 records: weights all 1, uniform in [0, 4096), the graph's own weights repeated, each
with the handling of equal values and without it (KATOME_SPECTRUM_PLAIN=1), and the stats call's weight pass over the same
array as the ceiling a histogram cannot pass.  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import katome_amd  # noqa: E402
from katome_amd import _lib  # noqa: E402
from katome_amd import device as kd  # noqa: E402
from katome_amd import workloads  # noqa: E402

HBM_PEAK = 8.0e12
BYTES = {"stats_degree_kernel": 32, "stats_weight_kernel": 4, "stats_node_kernel": 8, "spectrum_kernel": 4, "spectrum_kernel<plain>": 4}
TRACE = re.compile(r"\[katome_stats\] (\S+): ([0-9.]+) ms, (\d+) elements")


def traced(call):
    """call() with the process's stderr (the library's trace lines) kept in a file -> (result, [(kernel, ms, elements)])"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            res = call()
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    return res, [(m.group(1), float(m.group(2)), int(m.group(3))) for m in TRACE.finditer(text)]


def kernel_rows(lines):
    """per kernel: the best time over the launches seen, its bytes and its share of the HBM peak"""
    best = {}
    for name, ms, n in lines:
        if name not in best or ms < best[name][0]:
            best[name] = (ms, n)
    return {name: dict(ms=round(ms, 4), elements=n, bytes=n * BYTES[name], share_of_hbm_peak=round(n * BYTES[name] / (ms * 1e-3) / HBM_PEAK, 4) if ms else None)
            for name, (ms, n) in best.items()}


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def copy_out_route(b):
    """what the device calls replace: the three arrays to the host, then katome_graph_stats -> (d2h ms, host stats ms, stats)"""
    dg = b.graph()
    t0 = time.perf_counter()
    src, dst, w = dg.edge_src.cpu().numpy(), dg.edge_dst.cpu().numpy(), dg.edge_weight.cpu().numpy()
    t1 = time.perf_counter()
    g = _lib.Graph()
    g.n_nodes, g.n_edges = dg.n_nodes, dg.n_edges
    g.edge_src, g.edge_dst = src.ctypes.data_as(_lib.u64p), dst.ctypes.data_as(_lib.u64p)
    g.edge_weight = w.ctypes.data_as(_lib.u32p)
    st = _lib.Stats()
    assert katome_amd.lib().katome_graph_stats(C.byref(g), C.byref(st)) == 0
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, st


def measure_builder(b, bins, reps):
    calls = {"graph_stats": b.stats, "weight_spectrum": lambda: b.weight_spectrum(bins)}
    times = {name: [] for name in calls}
    times.update(copy_out_d2h=[], copy_out_host_stats=[])
    for rep in range(reps + 1):                              # (the first round warms up and is not kept; no trace: nothing waits inside a call)
        for name, call in calls.items():
            ms, res = wall(call)
            if rep:
                times[name].append(round(ms, 3))
            if name == "graph_stats":
                dev = res
        d2h, host, st = copy_out_route(b)
        if rep:
            times["copy_out_d2h"].append(round(d2h, 1)); times["copy_out_host_stats"].append(round(host, 1))
    os.environ["KATOME_STATS_TRACE"] = "1"                   # the kernels' own times, in a pass of their own
    lines = []
    for rep in range(reps):
        for call in calls.values():
            lines += traced(call)[1]
    del os.environ["KATOME_STATS_TRACE"]
    assert (dev.node_count, dev.edge_count, dev.max_edge_weight, dev.max_in_degree, dev.max_out_degree, dev.incoming_vert_count) == \
        (st.node_count, st.edge_count, st.max_edge_weight, st.max_in_degree, st.max_out_degree, st.incoming_vert_count)
    dg = b.graph()
    out = dict(edges=dg.n_edges, nodes=dg.n_nodes, bins=bins, call_ms=times, kernels=kernel_rows(lines),
               d2h_bytes=dg.n_edges * 20, max_edge_weight=dev.max_edge_weight, avg_edge_weight=dev.avg_edge_weight)
    best_dev = min(times["graph_stats"])
    best_copy = min(a + b_ for a, b_ in zip(times["copy_out_d2h"], times["copy_out_host_stats"]))
    out["copy_out_over_device"] = round(best_copy / best_dev, 1)
    out["spectrum_low_bins"] = [int(x) for x in b.weight_spectrum(bins)[:8]]
    return out


def build(wl, first_seen, prune):
    packed, skip = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, wl.n_inject_percent, device=0)
    skip_arg = skip if wl.n_inject_percent else None
    b = kd.Builder(wl.k, wl.reverse_complement, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2), first_seen_order=first_seen)
    step = 4 << 20
    for r0 in range(0, wl.reads, step):
        b.count_reads(packed, min(step, wl.reads - r0), wl.read_len, skip_arg, first_read=r0)
    b.finalize()
    if prune:
        b.remove_dead_paths()
    del packed, skip
    return b


def spectrum_alone(own_weights, bins, log2, reps):
    n = 1 << log2
    rng = torch.Generator(device="cuda").manual_seed(1)
    arrays = {"all 1": torch.ones(n, dtype=torch.int32, device="cuda"),
              "uniform in [0, 4096)": torch.randint(0, 4096, (n,), dtype=torch.int32, device="cuda", generator=rng),
              "the graph's own weights": own_weights.repeat((n + own_weights.numel() - 1) // own_weights.numel())[:n].contiguous()}
    ids = (torch.arange(n, dtype=torch.int64, device="cuda") & ((1 << 20) - 1))
    os.environ["KATOME_STATS_TRACE"] = "1"
    out = {}
    for rep in range(reps + 1):
        for name, w in arrays.items():
            row = out.setdefault(name, {})
            for plain in (False, True):
                if plain:
                    os.environ["KATOME_SPECTRUM_PLAIN"] = "1"
                _, seen = traced(lambda: kd.weight_spectrum_arrays(w, bins))
                os.environ.pop("KATOME_SPECTRUM_PLAIN", None)
                if rep:
                    row.setdefault("plain_ms" if plain else "handled_ms", []).append(round(sum(ms for _, ms, _ in seen), 4))
            _, seen = traced(lambda: kd.stats_arrays(ids, ids, w, 1 << 20))
            if rep:
                row.setdefault("weight_pass_ms", []).append(round(sum(ms for k, ms, _ in seen if k == "stats_weight_kernel"), 4))
    del os.environ["KATOME_STATS_TRACE"]
    for row in out.values():
        for key in ("handled_ms", "plain_ms", "weight_pass_ms"):
            row[key.replace("_ms", "_share_of_hbm_peak")] = round(n * 4 / (min(row[key]) * 1e-3) / HBM_PEAK, 4)
    return dict(records=n, bins=bins, cases=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--full", action="store_true", help="also C3 in full, by packed key")
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--records-log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    c3 = workloads.WORKLOADS["c3"]
    wl = c3.scaled(min(a.reads, c3.reads))
    out = dict(workload=wl.name, reads=wl.reads, k=wl.k, hbm_peak_bytes_per_s=HBM_PEAK)
    b = build(wl, True, True)
    try:
        out["first_seen_after_remove_dead_paths"] = measure_builder(b, a.bins, a.reps)
        own = b.graph().edge_weight.clone()
    finally:
        b.close()
    kd.release_cache(0)
    if a.records_log2:
        out["spectrum_kernel_alone"] = spectrum_alone(own, a.bins, a.records_log2, a.reps)
    del own
    if a.full:
        b = build(c3, False, False)
        try:
            out["c3_in_full_by_packed_key"] = measure_builder(b, a.bins, a.reps)
        finally:
            b.close()
    else:
        out["c3_in_full_by_packed_key"] = "not measured"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
