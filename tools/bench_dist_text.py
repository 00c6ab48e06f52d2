"""The end of the sharded pipeline on thread ranks that share this one GPU: per rank the text of the sharded shrink
(katome_dist_contigs_text: ms, bytes, GB/s), Contigs::stats of all ranks' contigs (katome_dist_contig_stats: ms) and the FASTA
file written by every rank (katome_dist_contigs_save: ms), on 2, 4 and 8 ranks, beside katome_dev_contigs_text of the same
contigs on one GPU.
usage: python tools/bench_dist_text.py [--reads 20000000] [--read-len 100] [--genome-len 5000000] [--k 31] [--ranks 2,4,8] [--reps 2]
                                       [--out /dev/shm/katome_unitigs.fa]

The ranks' exchanges are copies on one card and their kernels share it, so the numbers say what the calls cost in kernels and
collectives, nothing about scaling over GPUs: unmeasured on real links.  The per-rank lines are what KATOME_DIST_TEXT_TRACE
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

TRACE = re.compile(r"\[(katome_dist_contigs_text|katome_dist_contig_stats|katome_dist_contigs_save)\] rank (\d+)/(\d+): ([0-9.]+) ms, (\d+) bytes")


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
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "katome_unitigs.fa"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    packed_t, _ = kd.synth_reads(0, a.reads, a.read_len, a.genome_len, a.err, 0, device=0)
    packed = packed_t.cpu().numpy()
    n, L, k = a.reads, a.read_len, a.k
    out = dict(reads=n, read_len=L, k=k, genome_len=a.genome_len, err=a.err, ranks_share_one_gpu=True, links="unmeasured on real links", routes={})
    os.environ["KATOME_DIST_TEXT_TRACE"] = "1"

    def unitigs(n_dev):
        s = make_settings(k, reverse_complement=True, first_seen_order=True, n_devices=n_dev, ranks_share_device=n_dev > 1)
        u = _lib.Unitigs()
        st = _lib.lib().katome_unitigs_packed(C.byref(s), packed.ctypes.data, n, L, None, b"", a.genome_len, os.fsencode(a.out), C.byref(u))
        if st != 0:
            raise KatomePanic(st, _lib.last_error())
        return u

    for n_dev in [int(x) for x in a.ranks.split(",")]:
        best = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            u, err = captured_stderr(lambda: unitigs(n_dev))
            wall = (time.perf_counter() - t0) * 1e3
            per = {}
            for call, rank, _, ms, nbytes in TRACE.findall(err):
                per.setdefault(int(rank), {})[call] = (float(ms), int(nbytes))
            score = max(sum(v[0] for v in calls.values()) for calls in per.values())
            if best is None or score < best[0]:
                best = (score, wall, per, u)
        _, wall, per, u = best
        ranks = []
        for r in sorted(per):
            text_ms, text_bytes = per[r]["katome_dist_contigs_text"]
            ranks.append(dict(rank=r, text_ms=text_ms, text_bytes=text_bytes, text_GBps=text_bytes / (text_ms * 1e-3) / 1e9 if text_ms else 0.0,
                              stats_ms=per[r]["katome_dist_contig_stats"][0], save_ms=per[r]["katome_dist_contigs_save"][0]))
        out["routes"]["sharded/%d" % n_dev] = dict(ranks=n_dev, host_entry_ms=wall, contigs=u.n_contigs, text_bytes=u.text_bytes,
                                                   file_bytes=os.path.getsize(a.out), n50=u.stats.n50, l50=u.stats.l50, per_rank=ranks)
        print("[sharded/%d] host entry %.1f ms; %d contigs, %d bytes; per rank text/stats/save ms: %s" % (
            n_dev, wall, u.n_contigs, u.text_bytes, ", ".join("%.1f/%.1f/%.1f" % (x["text_ms"], x["stats_ms"], x["save_ms"]) for x in ranks)),
            file=sys.stderr, flush=True)
    # the same contigs on one GPU: katome_dev_contigs_text on a resident builder's fast shrink
    b = kd.Builder(k, True, first_seen_order=True)
    span = b.tile_span(L)
    pk = torch.cat([packed_t, torch.zeros(32, dtype=torch.uint8, device=packed_t.device)])
    if span > 1:
        b.insert_tiles(b.extract_tiles(pk, n, L, span), span)
    else:
        b.insert(b.extract_fixed(pk, n, L))
    b.finalize()
    dc = b.shrink(mode="fast")
    t = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        da = dc.text("fasta")
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
        nb, nc = da.text_bytes, da.n_contigs
        del da
    ms = min(t[1:])
    out["routes"]["one_gpu"] = dict(text_ms=ms, text_bytes=nb, contigs=nc, text_GBps=nb / (ms * 1e-3) / 1e9)
    print("[one GPU] katome_dev_contigs_text %.1f ms; %d contigs, %d bytes" % (ms, nc, nb), file=sys.stderr, flush=True)
    del dc
    b.close()
    if os.path.exists(a.out):
        os.remove(a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
