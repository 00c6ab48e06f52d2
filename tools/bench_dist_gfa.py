"""The unitig graph of the sharded shrink as GFA 1 on thread ranks that share this one GPU: per rank the join across ranks (wall
time, bytes sent), the numbered writer's kernels (their own time by HIP events, bytes, GB/s), the whole katome_dist_contigs_gfa
and the file written by every rank (katome_dist_gfa_save: ms), on 2, 4 and 8 ranks -- beside katome_dist_contigs_text of the
same shrink (the FASTA text: KATOME_DIST_TEXT_TRACE) and the one-GPU writer, k:gfa_write_kernel, on the same unitigs.
usage: python tools/bench_dist_gfa.py [--reads 20000000] [--read-len 100] [--genome-len 5000000] [--k 31] [--ranks 2,4,8] [--reps 2]
                                      [--out /dev/shm/katome_unitigs.gfa]

The ranks' exchanges are copies on one card and their kernels share it, so the numbers say what the calls cost in kernels and
collectives, nothing about scaling over GPUs: unmeasured on real links.  The per-rank lines are what KATOME_DIST_GFA_TRACE
reports (wall time of the whole call on that rank, its waits for the other ranks included); the best repetition is kept."""
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

GFA = re.compile(r"\[katome_dist_contigs_gfa\] rank (\d+)/\d+: ([0-9.]+) ms, (\d+) bytes, join ([0-9.]+) ms, (\d+) bytes sent, write ([0-9.]+) ms, (\d+) bytes")
SAVE = re.compile(r"\[katome_dist_gfa_save\] rank (\d+)/\d+: ([0-9.]+) ms, (\d+) bytes")
TEXT = re.compile(r"\[katome_dist_contigs_text\] rank (\d+)/\d+: ([0-9.]+) ms, (\d+) bytes")
ONE = re.compile(r"k:gfa_write_kernel ([0-9.]+) ms, (\d+) bytes, (\d+) segments, (\d+) links")


def captured_stderr(fn):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=float, default=1e-3)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--ranks", default="2,4,8")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "katome_unitigs.gfa"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    packed_t, _ = kd.synth_reads(0, a.reads, a.read_len, a.genome_len, a.err, 0, device=0)
    packed = packed_t.cpu().numpy()
    n, L, k = a.reads, a.read_len, a.k
    out = dict(reads=n, read_len=L, k=k, genome_len=a.genome_len, err=a.err, ranks_share_one_gpu=True, links="unmeasured on real links", routes={})
    os.environ["KATOME_DIST_GFA_TRACE"] = "1"
    os.environ["KATOME_DIST_TEXT_TRACE"] = "1"
    os.environ["KATOME_GFA_TRACE"] = "1"

    def run(n_dev, graph):
        s = make_settings(k, reverse_complement=True, first_seen_order=True, n_devices=n_dev, ranks_share_device=n_dev > 1)
        u = _lib.UnitigsGfa() if graph else _lib.Unitigs()
        fn = _lib.lib().katome_unitigs_gfa_packed if graph else _lib.lib().katome_unitigs_packed
        st = fn(C.byref(s), packed.ctypes.data, n, L, None, b"", a.genome_len, os.fsencode(a.out), C.byref(u))
        if st != 0:
            raise KatomePanic(st, _lib.last_error())
        return u

    for n_dev in [int(x) for x in a.ranks.split(",")]:
        best = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            u, err = captured_stderr(lambda: run(n_dev, True))
            wall = (time.perf_counter() - t0) * 1e3
            per = {int(m[0]): dict(rank=int(m[0]), gfa_ms=float(m[1]), join_ms=float(m[3]), join_bytes_sent=int(m[4]), write_ms=float(m[5]),
                                   write_bytes=int(m[6]), write_GBps=int(m[6]) / (float(m[5]) * 1e-3) / 1e9 if float(m[5]) else 0.0)
                   for m in GFA.findall(err)}
            for rank, ms, _ in SAVE.findall(err):
                per[int(rank)]["save_ms"] = float(ms)
            score = max(v["gfa_ms"] for v in per.values())
            if best is None or score < best[0]:
                best = (score, wall, per, u, os.path.getsize(a.out))
        _, wall, per, u, file_bytes = best
        _, err = captured_stderr(lambda: run(n_dev, False))         # the FASTA text of the same shrink, for the join's time to stand beside
        text_ms = {int(r): float(ms) for r, ms, _ in TEXT.findall(err)}
        ranks = [dict(per[r], fasta_text_ms=text_ms.get(r)) for r in sorted(per)]
        out["routes"]["sharded/%d" % n_dev] = dict(ranks=n_dev, host_entry_ms=wall, segments=u.n_segments, links=u.n_links, text_bytes=u.text_bytes,
                                                   file_bytes=file_bytes, per_rank=ranks)
        print("[sharded/%d] host entry %.1f ms; %d segments, %d links, %d bytes; per rank join/write/save ms (FASTA text ms): %s" % (
            n_dev, wall, u.n_segments, u.n_links, u.text_bytes,
            ", ".join("%.1f/%.3f/%.1f (%.1f)" % (x["join_ms"], x["write_ms"], x.get("save_ms", 0.0), x["fasta_text_ms"] or 0.0) for x in ranks)),
            file=sys.stderr, flush=True)
    # the same unitigs on one GPU: the resident builder's fast shrink through katome_dev_gfa_arrays, whose trace has the kernel's own time
    b = kd.Builder(k, True, first_seen_order=True)
    span = b.tile_span(L)
    pk = torch.cat([packed_t, torch.zeros(32, dtype=torch.uint8, device=packed_t.device)])
    if span > 1:
        b.insert_tiles(b.extract_tiles(pk, n, L, span), span)
    else:
        b.insert(b.extract_fixed(pk, n, L))
    b.finalize()
    dc = b.shrink(mode="fast")
    times = []
    for _ in range(a.reps + 1):
        g, err = captured_stderr(lambda: kd.gfa_arrays(k, dc.n_nodes, dc.edge_src, dc.edge_dst, dc.edge_weight, dc.edge_kmers, dc.edge_label_off, dc.edge_label,
                                                       label_bytes=dc.label_bytes))
        m = ONE.search(err)
        times.append((float(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))))
        del g
    ms, nb, ns, nl = min(times[1:])
    out["routes"]["one_gpu"] = dict(write_ms=ms, text_bytes=nb, segments=ns, links=nl, write_GBps=nb / (ms * 1e-3) / 1e9)
    print("[one GPU] k:gfa_write_kernel %.4f ms; %d segments, %d links, %d bytes" % (ms, ns, nl, nb), file=sys.stderr, flush=True)
    del dc
    b.close()
    if os.path.exists(a.out):
        os.remove(a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
