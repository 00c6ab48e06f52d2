"""The sharded build of reads of varying length against reads of one length with the same windows in all.
usage: python tools/bench_dist_var.py [--reads 400000] [--k 31] [--ranks 4] [--reps 5] [--exchange-ranks 2] [--out result.json]

Wall time of katome_build_files (GpuGraph.create with n_devices, every repetition) for a FASTQ of reads whose lengths are drawn from 100..150
and for one of 125-base reads with the same total number of windows, on the "local" and "tiles" routes, by packed key and in
first-seen order.  The ranks are threads that share this one GPU (ranks_share_device): the numbers say what the route costs in
kernels and exchanges on one card, nothing about scaling over GPUs.  The time includes parsing the FASTQ on the host.
Then the exchange bytes per rank: --exchange-ranks processes (katome_amd/launch.py) share the card, their exchanges go through
gloo, each builds its share of the same reads on the tiles route through add_reads_var and through add_reads, by packed key and
in first-seen order, and reads ShardedBuilder.exchange_stats(): what the 16-byte sequence numbers of the variable-length records
cost against the 4-byte index of fixed-length ones."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from katome_amd import shard as ks  # noqa: E402
from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes  # noqa: E402


def write_fastq(path, genome, lens, rng):
    with open(path, "w") as f:
        for i, L in enumerate(lens):
            at = int(rng.integers(0, len(genome) - L))
            s = genome[at:at + L]
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * L))


def timed_build(path, k, ranks, first_seen, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        g, _ = GpuGraph.create([path], InputFileType.Fastq, True, 0, first_seen_order=first_seen, n_devices=ranks, ranks_share_device=True)
        times.append((time.perf_counter() - t) * 1e3)
        n_edges = g.n_edges
        del g
    return times, n_edges


def exchange_reads(k, n, seed=7, genome_len=1_000_000, fixed_len=125):
    """the reads of the exchange measurement: n of lengths 100..150, and reads of fixed_len with the same windows"""
    rng = np.random.default_rng(seed)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, genome_len))
    lens = rng.integers(100, 151, n)
    var = [genome[a:a + int(L)] for a, L in zip(rng.integers(0, genome_len - 151, n), lens)]
    nf = int((lens - k + 1).sum()) // (fixed_len - k + 1)
    fixed = [genome[a:a + fixed_len] for a in rng.integers(0, genome_len - fixed_len, nf)]
    return var, fixed


def exchange_child(out_dir, k, n):
    """one rank of the exchange measurement (started by launch_ranks)"""
    import torch.distributed as dist
    from tests.helpers import pack_reads_ascii
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        os.environ["KATOME_DIST_ROUTE"] = "tiles"
        var, fixed = exchange_reads(k, n)
        comm = ks.Comm.over_torch(device=0)
        out = {}
        for fs in (False, True):
            for name, reads in (("var", var), ("fixed", fixed)):
                first, count = ks.shard_range(len(reads), world, rank)
                mine = reads[first:first + count]
                b = ks.ShardedBuilder(comm, k, True, 0, first_seen_order=fs)
                if name == "var":
                    packed = [pack_reads_ascii(np.frombuffer(s.encode(), np.uint8)[None, :]).reshape(-1) for s in mine]
                    off = np.concatenate([[0], np.cumsum([len(p) for p in packed])]).astype(np.int64)
                    lens = np.array([len(s) for s in mine], np.int32)
                    b.add_reads_var(torch.from_numpy(np.concatenate(packed + [np.zeros(32, np.uint8)])).cuda(), torch.from_numpy(off).cuda(),
                                    torch.from_numpy(lens).cuda())
                else:
                    L = len(reads[0])
                    packed = pack_reads_ascii(np.frombuffer("".join(mine).encode(), np.uint8).reshape(len(mine), L)).reshape(-1)
                    b.add_reads(torch.from_numpy(np.concatenate([packed, np.zeros(32, np.uint8)])).cuda(), first, len(mine), L)
                b.finalize()
                out["%s/%s" % ("first_seen" if fs else "packed", name)] = {p: x["bytes_out"] for p, x in b.exchange_stats().items()}
                b.close()
        comm.close()
        with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


def exchange_bytes(world, k, n):
    from katome_amd.launch import launch_ranks
    with tempfile.TemporaryDirectory() as d:
        code, _ = launch_ranks(world, [sys.executable, os.path.abspath(__file__), "--exchange-child", d, "--k", str(k),
                                       "--exchange-reads", str(n)], timeout=600)
        if code != 0:
            raise SystemExit("exchange ranks failed: exit %d" % code)
        return [json.load(open(os.path.join(d, "rank%d.json" % r))) for r in range(world)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=400_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--out", default="")
    ap.add_argument("--exchange-ranks", type=int, default=2)
    ap.add_argument("--exchange-reads", type=int, default=100_000)
    ap.add_argument("--exchange-child", default="")
    a = ap.parse_args()
    if a.exchange_child:
        exchange_child(a.exchange_child, a.k, a.exchange_reads)
        return
    rng = np.random.default_rng(1)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, a.genome_len))
    lens = rng.integers(100, 151, a.reads)
    windows = int((lens - a.k + 1).sum())
    fixed_len = 125
    n_fixed = windows // (fixed_len - a.k + 1)
    set_global_k_sizes(a.k)
    res = dict(reads_var=a.reads, reads_fixed=n_fixed, windows=windows, k=a.k, ranks=a.ranks, reps=a.reps, builds={})
    with tempfile.TemporaryDirectory() as d:
        pv, pf = os.path.join(d, "var.fq"), os.path.join(d, "fixed.fq")
        write_fastq(pv, genome, lens.tolist(), rng)
        write_fastq(pf, genome, [fixed_len] * n_fixed, rng)
        for route in ("local", "tiles"):
            os.environ["KATOME_DIST_ROUTE"] = route
            for fs in (False, True):
                for name, path in (("var", pv), ("fixed", pf)):
                    times, ne = timed_build(path, a.k, a.ranks, fs, a.reps)
                    res["builds"]["%s/%s/%s" % (route, "first_seen" if fs else "packed", name)] = dict(
                        ms_min=round(min(times), 1), ms_max=round(max(times), 1), edges=ne)
                    print(route, fs, name, [round(t, 1) for t in times], ne, flush=True)
        os.environ.pop("KATOME_DIST_ROUTE", None)
    if a.exchange_ranks > 1:
        res["exchange_bytes_per_rank"] = exchange_bytes(a.exchange_ranks, a.k, a.exchange_reads)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
