"""remove_dead_paths on the sharded graph, the ranks as threads that share this one GPU: one build in first-seen order with
KATOME_FLAG_REMOVE_DEAD_PATHS, the library's own `[dist prune]` lines left on stderr (tools/bench_dist_shrink.py captures them).
usage: KATOME_DIST_PRUNE_TRACE=1 [KATOME_DIST_PRUNE_WALKS=table|hop] [KATOME_TRACE_BLOCKS=1] python tools/bench_dist_prune.py
           [--reads 5000000] [--read-len 100] [--genome-len 2000000] [--err 1e-3] [--k 31] [--ranks 4]
The library reads KATOME_DIST_PRUNE_TRACE once per process: set it in the environment, one process per measurement.  Prints the
wall time of the whole entry (build + pruning + the result in host arrays), the pruned graph's size and the device pool's size."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from katome_amd import device as kd  # noqa: E402
from katome_amd.build import GpuGraph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--err", type=float, default=1e-3)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--ranks", type=int, default=4)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    packed_t, _ = kd.synth_reads(0, a.reads, a.read_len, a.genome_len, a.err, 0, device=0)
    packed = packed_t.cpu().numpy()
    del packed_t
    t0 = time.perf_counter()
    g, _ = GpuGraph.create_from_packed(packed, a.reads, a.read_len, reverse_complement=True, k=a.k, n_devices=a.ranks, ranks_share_device=True,
                                       first_seen_order=True, remove_dead_paths=True)
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(lib=os.environ.get("KATOME_LIB", "tree"), ranks=a.ranks, reads=a.reads, ms=ms, edges=g.n_edges, nodes=g.n_nodes,
                          edge_sum=int(g.edge_src.sum() + g.edge_dst.sum()), cache=kd.cache_stats(0))))


if __name__ == "__main__":
    main()
