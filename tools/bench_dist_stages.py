"""The stages before collapse ("dcwced") on the sharded graph, on the gathered graph and on one GPU: wall time of each stage.
usage: python tools/bench_dist_stages.py [--reads 10000000] [--read-len 250] [--genome-len 20000000] [--ranks 4] [--reps 2]
                                       [--stages dcwced]

A first-seen k = 63 build of synthetic reads (BASELINE config 5's k and error rate) through katome_build_packed_staged with
the stage strings "", "d", "dc", ... "dcwced"; a stage's time is the difference between the best runs of two consecutive
prefixes, so it includes the change in the time the result takes to reach the host arrays.  The ranks are threads that
share this one GPU (ranks_share_device): the numbers say what the sharded route costs in kernels and exchanges on one
card, nothing about scaling over GPUs or about real links."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from katome_amd import device as kd  # noqa: E402
from katome_amd import workloads  # noqa: E402
from katome_amd.build import GpuGraph  # noqa: E402

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=2)
    ap.add_argument("--read-len", type=int, default=250)
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--stages", default="dcwced", help="the stage string whose prefixes are timed")
    a = ap.parse_args()
    STAGES = a.stages
    c5 = workloads.WORKLOADS["c5"]
    wl = workloads.Workload("c5-shape/%d" % a.reads, a.reads, a.read_len, c5.k, a.genome_len, c5.err_rate, c5.n_inject_percent)
    torch.cuda.set_device(0)
    packed, skip = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, wl.n_inject_percent, device=0)
    packed = packed.cpu().numpy()
    skip = skip[:wl.reads].cpu().numpy() if wl.n_inject_percent else None
    glen = wl.genome_len
    out = dict(workload=wl.name, reads=wl.reads, read_len=wl.read_len, k=wl.k, stages=STAGES, ranks=a.ranks, threshold=a.threshold, genome_len=glen,
               ranks_share_one_gpu=True, routes={})
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
