"""Times what unitig coverage costs, and that it costs nothing where it is not asked for:
    python tools/bench_coverage.py [--reads 20000000] [--exact-reads 2000000] [--dist-reads 2000000] [--runs 3] [--parent-lib PATH/libkatome_gpu.so]
-> one JSON line

The input is a by-key build of C3's first --reads reads (150 bp, k = 31, both strands).  A library is loaded once per process, so
every variant runs in a child process of its own (`--child`), the children of the two libraries alternating; a child builds the graph,
warms every call up once and then alternates the calls it times --runs times:
  * katome_dev_shrink_mode(FAST) / katome_dev_shrink_coverage(FAST): wall time around the call (it ends in a device synchronise);
  * the EXACT pair on a first-seen build of the first --exact-reads reads after the first pruning (tools/time_shrink.py's graph; the
    host walk takes 87 ns per edge, so the size is kept apart): wall time, the host walk (host_ms) and the device part, their difference;
  * katome_dev_contigs_gfa / katome_dev_contigs_gfa_coverage: wall time and, from the phase table, "k:gfa sizes" and
    "k:gfa_write_kernel" with the bytes written;
  * (this tree's library only) the sharded pair on 8 thread ranks sharing the card, --dist-reads reads, through
    katome_unitigs_gfa_packed with and without KATOME_FLAG_PATH_COVERAGE: every rank's katome_dist_shrink time and bytes sent, from
    KATOME_DIST_SHRINK_TRACE.
With --parent-lib the plain calls are also timed on that library (the parent commit's, built beside this one): "no request, no cost"
holds when the two medians differ by less than the two spreads.  Per quantity: the median and (min, max) over the runs.
A kernel-level view (path_measure_kernel beside path_write_kernel with and without coverage: what a separate coverage walk would
cost at the least) comes from running one child under rocprofv3 --kernel-trace --stats:  ... -- python tools/bench_coverage.py --child one"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=20_000_000)
ap.add_argument("--exact-reads", type=int, default=2_000_000)
ap.add_argument("--dist-reads", type=int, default=2_000_000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--child", choices=["one", "dist"], default=None)
ap.add_argument("--plain-only", action="store_true", help="(child) the library has no coverage entries: the parent's")
args = ap.parse_args()


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) * 1e3


def build(first_seen, reads):
    from katome_amd import device as kd
    from katome_amd.workloads import WORKLOADS
    w = WORKLOADS["c3"].scaled(reads)
    packed, skip = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, 0, device=0)
    b = kd.Builder(w.k, True, table_slots_hint=int(w.expected_distinct_canonical() * 2.2), first_seen_order=first_seen)
    step = 4 << 20
    for r0 in range(0, w.reads, step):
        b.count_reads(packed, min(step, w.reads - r0), w.read_len, None, first_read=r0)
    dg = b.finalize()
    info = {"reads": w.reads, "k": w.k, "edges": dg.n_edges, "nodes": dg.n_nodes}
    del dg, packed, skip
    return b, info


def child_one():
    """one GPU: the fast pair and the GFA pair on the by-key build, the exact pair on the pruned first-seen build"""
    cov = not args.plain_only
    b, out = build(False, args.reads)
    variants = [False, True] if cov else [False]
    runs = {}
    b.profile(True)
    for run in range(args.runs + 1):               # (run 0: warm-up)
        for c in variants:
            tag = "coverage" if c else "plain"
            b.profile_read()
            dc, ms = timed(lambda: b.shrink("fast", coverage=True) if c else b.shrink("fast"))
            b.profile_read()
            g, gms = timed(lambda: dc.gfa(coverage=True) if c else dc.gfa())
            prof = b.profile_read()
            out.setdefault("segments", dc.n_edges)
            out["gfa_bytes_" + tag] = g.text_bytes
            if run:
                for name, v in (("shrink_fast_ms", ms), ("gfa_wall_ms", gms), ("gfa_sizes_ms", prof["k:gfa sizes"][0]), ("gfa_write_ms", prof["k:gfa_write_kernel"][0])):
                    runs.setdefault("%s_%s" % (name, tag), []).append(v)
            del g, dc
    b.close()
    b, info = build(True, args.exact_reads)
    dg, _ = b.remove_dead_paths()
    out["exact_reads"], out["edges_after_pruning"] = info["reads"], dg.n_edges
    del dg
    for run in range(args.runs + 1):
        for c in variants:
            tag = "coverage" if c else "plain"
            dc, ms = timed(lambda: b.shrink("exact", coverage=True) if c else b.shrink("exact"))
            host = b.last_shrink_host_ms
            out.setdefault("segments_exact", dc.n_edges)
            del dc
            if run:
                for name, v in (("shrink_exact_ms", ms), ("shrink_exact_host_ms", host), ("shrink_exact_device_ms", ms - host)):
                    runs.setdefault("%s_%s" % (name, tag), []).append(v)
    b.close()
    out.update({k: spread(v) for k, v in runs.items()})
    print("RESULT " + json.dumps(out), flush=True)


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


def child_dist():
    """8 thread ranks on one card: katome_unitigs_gfa_packed with and without the flag; the ranks' shrink lines of the trace"""
    os.environ["KATOME_DIST_SHRINK_TRACE"] = "1"
    import numpy as np
    from katome_amd import device as kd
    from katome_amd.build import GpuUnitigs
    from katome_amd.workloads import WORKLOADS
    w = WORKLOADS["c3"].scaled(args.dist_reads)
    packed, skip = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, 0, device=0)
    host = packed.cpu().numpy()
    del packed, skip
    out, runs = {"dist_reads": w.reads, "ranks": 8}, {}
    for run in range(args.runs + 1):
        for c in (False, True):
            tag = "coverage" if c else "plain"
            (u, _), err = traced(lambda: GpuUnitigs.gfa_from_packed(host, w.reads, w.read_len, reverse_complement=True, k=w.k, n_devices=8,
                                                                    ranks_share_device=True, coverage=c))
            lines = re.findall(r"\[katome_dist_shrink\] rank (\d+)/8: ([0-9.]+) ms, .*? sent (\d+) bytes", err)
            assert len(lines) == 8, err
            out["dist_segments"] = u.n_segments
            out["dist_bytes_sent_per_rank_" + tag] = [int(n) for _, _, n in sorted(lines, key=lambda x: int(x[0]))]
            if run:
                runs.setdefault("dist_shrink_slowest_rank_ms_" + tag, []).append(max(float(ms) for _, ms, _ in lines))
    out.update({k: spread(v) for k, v in runs.items()})
    out["dist_bytes_sent_ratio"] = sum(out["dist_bytes_sent_per_rank_coverage"]) / max(1, sum(out["dist_bytes_sent_per_rank_plain"]))
    print("RESULT " + json.dumps(out), flush=True)


if args.child and args.plain_only:                 # the parent's library: bind what it has (it lacks exactly the coverage entries)
    import ctypes
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch brought, as in every other process here)
    from katome_amd import _lib
    _parent = ctypes.CDLL(_lib.lib_path())
    for _name in [n for n in _lib.SYMBOLS if not hasattr(_parent, n)]:
        assert _name.endswith("_coverage") or "_coverage_" in _name, _name
        del _lib.SYMBOLS[_name]
if args.child == "one":
    child_one()
    sys.exit(0)
if args.child == "dist":
    child_dist()
    sys.exit(0)


def run_child(kind, lib, plain_only=False):
    env = dict(os.environ)
    if lib:
        env["KATOME_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--reads", str(args.reads), "--exact-reads", str(args.exact_reads), "--dist-reads", str(args.dist_reads), "--runs", str(args.runs)]
    if plain_only:
        cmd.append("--plain-only")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit("child %s failed with status %d" % (kind, p.returncode))
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:])


out = {"this": [], "parent": []}
for i in range(args.runs if args.parent_lib else 1):          # the two libraries alternate, each child timing its own --runs runs
    if args.parent_lib:
        out["parent"].append(run_child("one", args.parent_lib, plain_only=True))
    out["this"].append(run_child("one", None))
out["dist"] = run_child("dist", None)
if args.parent_lib:
    for name in ("shrink_fast_ms_plain", "gfa_wall_ms_plain", "gfa_sizes_ms_plain", "gfa_write_ms_plain"):
        both = {side: [r[name]["median"] for r in out[side]] for side in ("this", "parent")}
        lo = {side: min(r[name]["min"] for r in out[side]) for side in both}
        hi = {side: max(r[name]["max"] for r in out[side]) for side in both}
        med = {side: statistics.median(both[side]) for side in both}
        out["no_cost_" + name] = {"this": [med["this"], lo["this"], hi["this"]], "parent": [med["parent"], lo["parent"], hi["parent"]],
                                  "difference": med["this"] - med["parent"], "within_spreads": abs(med["this"] - med["parent"]) <= (hi["this"] - lo["this"]) + (hi["parent"] - lo["parent"])}
print(json.dumps(out), flush=True)
