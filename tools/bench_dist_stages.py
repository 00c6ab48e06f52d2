"""The stages before collapse ("dcwced") on the sharded graph, on the gathered graph and on one GPU: wall time of each stage.
usage: python tools/bench_dist_stages.py [--reads 10000000] [--read-len 250] [--genome-len 20000000] [--ranks 4] [--reps 2]
                                       [--stages dcwced] [--contigs-route table|ranked] [--contigs-ab RUNS]

A first-seen k = 63 build of synthetic reads (BASELINE config 5's k and error rate) through katome_build_packed_staged with
the stage strings "", "d", "dc", ... "dcwced"; a stage's time is the difference between the best runs of two consecutive
prefixes, so it includes the change in the time the result takes to reach the host arrays.  The ranks are threads that
share this one GPU (ranks_share_device): the numbers say what the sharded route costs in kernels and exchanges on one
card, nothing about scaling over GPUs or about real links.

--contigs-route names the route of the sharded standardize_contigs for the whole run (KATOME_DIST_CONTIGS).  --contigs-ab RUNS
times that stage alone on both routes instead: sharded builds with the stage string --stages (give one that ends with the
'c' to time, e.g. "c"), the routes alternated, RUNS calls each, with KATOME_DIST_CONTIGS_TRACE on, which the tool reads back: the
JSON line carries, per call, the stage's own wall time (the slowest rank), its rounds, exchanges and bytes, and the whole call's
wall time beside it."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from katome_amd import device as kd  # noqa: E402
from katome_amd import workloads  # noqa: E402
from katome_amd.build import GpuGraph  # noqa: E402

TRACE = re.compile(r"\[katome_dist_standardize_contigs\] rank (\d+)/(\d+): ([0-9.]+) ms, route (\w+), ranking rounds (\d+), exchanges (\d+), "
                   r"contigs (\d+), longest (\d+), cycle edges (\d+), sent (\d+) bytes")


def traced(call):
    """call() with the process's stderr (file descriptor 2: the library's trace lines) kept in a file -> (result, text)"""
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
    sys.stderr.write(text)
    return res, text


def contigs_ab(a, wl, packed, skip, glen):
    """the last 'c' of --stages on both routes, alternated, --contigs-ab calls each after one warm-up pair: the stage's own
    wall time as the library's trace gives it (the slowest rank of the call's last standardize_contigs), its rounds,
    exchanges and bytes, and the wall time of the whole call beside it"""
    os.environ["KATOME_DIST_STAGES"] = "sharded"
    os.environ["KATOME_DIST_CONTIGS_TRACE"] = "1"
    runs = {"table": [], "ranked": []}
    sizes = {}
    for run in range(a.contigs_ab + 1):
        for route in ("table", "ranked"):
            os.environ["KATOME_DIST_CONTIGS"] = route
            t0 = time.perf_counter()
            (g, _), text = traced(lambda: GpuGraph.create_from_packed(
                packed, wl.reads, wl.read_len, skip=skip, reverse_complement=wl.reverse_complement, k=wl.k, first_seen_order=True,
                n_devices=a.ranks, ranks_share_device=True, stages=a.stages, original_genome_length=glen,
                minimal_weight_threshold=a.threshold))
            call_ms = (time.perf_counter() - t0) * 1e3
            sizes = dict(edges=g.n_edges, nodes=g.n_nodes)
            del g
            lines = [m.groups() for m in TRACE.finditer(text)][-a.ranks:]
            if len(lines) != a.ranks or any(l[3] != route for l in lines):
                raise SystemExit("no trace line of every rank for route %s:\n%s" % (route, text))
            rec = dict(stage_ms=round(max(float(l[2]) for l in lines), 2), call_ms=round(call_ms, 1), rank_rounds=int(lines[0][4]),
                       exchanges=int(lines[0][5]), contigs=int(lines[0][6]), longest_contig=int(lines[0][7]), cycle_edges=int(lines[0][8]),
                       bytes_sent_per_rank=[int(l[9]) for l in sorted(lines, key=lambda l: int(l[0]))])
            print("[contigs-ab] run %d %-6s stage %.1f ms, call %.1f ms" % (run, route, rec["stage_ms"], call_ms), file=sys.stderr, flush=True)
            if run:                                             # (the first pair warms up and is not kept)
                runs[route].append(rec)
    summary = {}
    for route, recs in runs.items():
        ms = sorted(r["stage_ms"] for r in recs)
        summary[route] = dict(stage_ms_median=ms[len(ms) // 2], stage_ms_min=ms[0], stage_ms_max=ms[-1])
    return dict(sizes, contigs_ab=runs, contigs_ab_summary=summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=2)
    ap.add_argument("--read-len", type=int, default=250)
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--stages", default="dcwced", help="the stage string whose prefixes are timed")
    ap.add_argument("--contigs-route", choices=("table", "ranked"), default=None, help="KATOME_DIST_CONTIGS for the whole run")
    ap.add_argument("--contigs-ab", type=int, default=0, metavar="RUNS", help="alternate the two routes of standardize_contigs, RUNS calls each")
    a = ap.parse_args()
    STAGES = a.stages
    if a.contigs_route:
        os.environ["KATOME_DIST_CONTIGS"] = a.contigs_route
    c5 = workloads.WORKLOADS["c5"]
    wl = workloads.Workload("c5-shape/%d" % a.reads, a.reads, a.read_len, c5.k, a.genome_len, c5.err_rate, c5.n_inject_percent)
    torch.cuda.set_device(0)
    packed, skip = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, wl.n_inject_percent, device=0)
    packed = packed.cpu().numpy()
    skip = skip[:wl.reads].cpu().numpy() if wl.n_inject_percent else None
    glen = wl.genome_len
    out = dict(workload=wl.name, reads=wl.reads, read_len=wl.read_len, k=wl.k, stages=STAGES, ranks=a.ranks, threshold=a.threshold, genome_len=glen,
               ranks_share_one_gpu=True, routes={})
    if a.contigs_ab:
        out.update(contigs_ab(a, wl, packed, skip, glen))
        del out["routes"]
        print(json.dumps(out))
        return
    for route, n_dev in (("sharded", a.ranks), ("gather", a.ranks), ("one_gpu", 1)):
        os.environ["KATOME_DIST_STAGES"] = "sharded" if route == "sharded" else "gather"
        best, sizes = [], []
        for i in range(len(STAGES) + 1):
            prefix = STAGES[:i]
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                g, _ = GpuGraph.create_from_packed(packed, wl.reads, wl.read_len, skip=skip, reverse_complement=wl.reverse_complement,
                                                   k=wl.k, first_seen_order=True, n_devices=n_dev, ranks_share_device=n_dev > 1,
                                                   stages=prefix or None, original_genome_length=glen,
                                                   minimal_weight_threshold=a.threshold)
                t.append((time.perf_counter() - t0) * 1e3)
                n = (g.n_edges, g.n_nodes)
                del g
            best.append(min(t))
            sizes.append(n)
            print("[%s] %-7s %9.1f ms  edges %d nodes %d" % (route, prefix or "build", best[-1], n[0], n[1]), file=sys.stderr, flush=True)
        out["routes"][route] = dict(build_ms=round(best[0], 1),
                                    stage_ms=[[STAGES[i], round(best[i + 1] - best[i], 1)] for i in range(len(STAGES))],
                                    edges_after=[s[0] for s in sizes], nodes_after=[s[1] for s in sizes])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
