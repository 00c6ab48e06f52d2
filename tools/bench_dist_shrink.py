"""Three ways to shrink a first-seen build after remove_dead_paths: the sharded shrink (katome_dist_shrink) on 2, 4 and 8
ranks, the gather followed by the fast form on the first GPU, and the one-GPU fast form.
usage: python tools/bench_dist_shrink.py [--reads 20000000] [--read-len 100] [--genome-len 5000000] [--k 31] [--ranks 2,4,8]
                                        [--reps 2] [--no-dead-paths]

The ranks are threads that share this one GPU (ranks_share_device): their exchanges are copies on one card, so the numbers
say what the sharded route costs in kernels and exchange calls, nothing about scaling over GPUs or about real links.
Per route: the best wall time of katome_shrink_packed (build + remove_dead_paths + shrink + the result in host arrays) and
what KATOME_DIST_SHRINK_TRACE reports -- for the sharded route every rank's katome_dist_shrink (ms, ranking rounds, bytes
sent), for the gathered one rank 0's gather + fast form + copy to host arrays (with remove_dead_paths: the pruning too, which
then runs on the gathered graph).  The one-GPU fast form is timed alone on a resident builder."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from katome_amd import device as kd  # noqa: E402
from katome_amd import _lib  # noqa: E402
from katome_amd.build import KatomePanic, make_settings  # noqa: E402

GATHER = re.compile(r"\[katome_dist_shrink\] gather \+ fast form on rank 0: ([0-9.]+) ms")
TRACE = re.compile(r"\[katome_dist_shrink\] rank (\d+)/(\d+): ([0-9.]+) ms, ranking rounds (\d+), cycle rounds (\d+), longest path (\d+), sent (\d+) bytes")


def captured_stderr(fn):
    """fn()'s result and what the library wrote to fd 2 meanwhile"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def best_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=float, default=1e-3)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--ranks", default="2,4,8")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-dead-paths", action="store_true", help="shrink the graph as built (remove_dead_paths leaves little of a clean genome)")
    a = ap.parse_args()
    dead = not a.no_dead_paths
    torch.cuda.set_device(0)
    packed_t, _ = kd.synth_reads(0, a.reads, a.read_len, a.genome_len, a.err, 0, device=0)
    packed = packed_t.cpu().numpy()
    n, L, k = a.reads, a.read_len, a.k
    out = dict(reads=n, read_len=L, k=k, genome_len=a.genome_len, err=a.err, remove_dead_paths=dead, ranks_share_one_gpu=True, routes={})

    class Shrunk:
        def __init__(self, c):
            self.n_edges, self.n_nodes = c.n_edges, c.n_nodes

    def contigs(n_dev):
        """katome_shrink_packed; only the sizes are read (decoding millions of labels in Python would time Python)"""
        s = make_settings(k, reverse_complement=True, first_seen_order=True, remove_dead_paths=dead, n_devices=n_dev,
                          ranks_share_device=n_dev > 1)
        cp = C.POINTER(_lib.Contigs)()
        st = _lib.lib().katome_shrink_packed(C.byref(s), packed.ctypes.data, n, L, None, C.byref(cp))
        if st != 0:
            raise KatomePanic(st, _lib.last_error())
        out = Shrunk(cp.contents)
        _lib.lib().katome_contigs_free(cp)
        return out

    for n_dev in [int(x) for x in a.ranks.split(",")]:
        for route in ("sharded", "gather"):
            os.environ["KATOME_DIST_SHRINK"] = route
            os.environ["KATOME_DIST_SHRINK_TRACE"] = "1"
            t_all, (c, err) = best_ms(lambda: captured_stderr(lambda: contigs(n_dev)), a.reps)
            del os.environ["KATOME_DIST_SHRINK_TRACE"]
            ranks = [dict(rank=int(m[0]), ms=float(m[2]), rank_rounds=int(m[3]), cycle_rounds=int(m[4]), longest_path=int(m[5]), bytes_sent=int(m[6]))
                     for m in TRACE.findall(err)][-n_dev:]
            gathered = [float(x) for x in GATHER.findall(err)]
            r = dict(ranks=n_dev, host_entry_ms=t_all, merged_edges=c.n_edges, merged_nodes=c.n_nodes, per_rank=ranks,
                     gather_fast_ms=min(gathered) if gathered else None)
            out["routes"]["%s/%d" % (route, n_dev)] = r
            line = "[%s/%d] host entry %.1f ms; merged edges %d" % (route, n_dev, r["host_entry_ms"], c.n_edges)
            if gathered:
                line += "; gather + fast form on rank 0: %.1f ms" % min(gathered)
            if ranks:
                line += "; shrink per rank: " + ", ".join("%.1f ms %d rounds %.1f MB" % (x["ms"], x["rank_rounds"], x["bytes_sent"] / 1e6) for x in ranks)
            print(line, file=sys.stderr, flush=True)
    os.environ.pop("KATOME_DIST_SHRINK", None)
    # the one-GPU fast form alone, on a resident builder after remove_dead_paths
    b = kd.Builder(k, True, first_seen_order=True)
    span = b.tile_span(L)
    pk = torch.cat([packed_t, torch.zeros(32, dtype=torch.uint8, device=packed_t.device)])
    if span > 1:
        b.insert_tiles(b.extract_tiles(pk, n, L, span), span)
    else:
        b.insert(b.extract_fixed(pk, n, L))
    b.finalize()
    if dead:
        b.remove_dead_paths()
    t = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dc = b.shrink(mode="fast")
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
        ne = dc.n_edges
        del dc
    out["routes"]["one_gpu_fast"] = dict(shrink_ms=min(t[1:]), merged_edges=ne)
    print("[one GPU] fast shrink %.1f ms; merged edges %d" % (min(t[1:]), ne), file=sys.stderr, flush=True)
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
