"""First-seen builds of trimmed reads: the levels counted by sorting (KATOME_SEEN_VAR_SORTED=1) against the HBM tables (=0).
usage: python tools/bench_var_seen.py [--reads 20000000] [--ks 31,40] [--reps 3] [--out profiles/r19_var_seen.md]

Input: c3's synthetic reads (katome_amd/workloads.py, genome scaled with the read count, no injected N) trimmed to lengths drawn
from 100..150, generated and kept on the device; first-seen order, both strands.  Every measurement is one build in a fresh child
process (the switch is read once per process), the two settings alternated --reps times after one discarded run: wall time of the batches + finalize, and the
per-phase times of katome_builder_profile.  Both settings run this library, so =0 is the route every such build took before; the
children also print a digest of the graph's arrays, which has to agree between the two.  Writes a markdown report."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(k, reads):
    import numpy as np
    import torch
    from katome_amd import device as kd
    from katome_amd.workloads import WORKLOADS
    w = WORKLOADS["c3"].scaled(reads)
    packed, _ = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, 0)
    lens_h = np.random.default_rng(19).integers(100, 151, w.reads).astype(np.int32)       # trimmed: the first len bases of every read
    lens = torch.from_numpy(lens_h).cuda()
    byte_off = (torch.arange(w.reads + 1, dtype=torch.int64) * w.stride).cuda()
    span = kd.tile_span_for_lengths(k, lens_h)
    batch = 1 << 28                                    # windows per batch
    warm = kd.Builder(k, True, first_seen_order=True)  # (code objects loaded, the allocator's first blocks)
    n0 = min(w.reads, 100000)
    warm.count_var_reads(packed, byte_off[:n0 + 1], lens[:n0], span=span)
    warm.finalize()
    warm.close()
    b = kd.Builder(k, True, first_seen_order=True)
    b.profile(True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    b.count_var_reads(packed, byte_off, lens, span=span, batch_windows=batch)
    dg = b.finalize()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    phases = {name: round(v[0], 3) for name, v in b.profile_read().items() if not name.startswith("k:")}
    h = hashlib.sha256()                               # of position-weighted sums taken on the device (the arrays are gigabytes)
    for a in (dg.edge_label, dg.edge_weight, dg.edge_src, dg.edge_dst):
        flat = a.reshape(-1).to(torch.int64)
        pos = torch.arange(flat.numel(), dtype=torch.int64, device=flat.device) % 1000003 + 1
        h.update(str(int((flat * pos).sum().item())).encode())
    print("RESULT " + json.dumps(dict(k=k, reads=reads, span=span, wall_ms=round(wall, 2), phases=phases, counts=b.counts(), n_edges=dg.n_edges,
                                      digest=h.hexdigest()[:16], sorted=os.environ.get("KATOME_SEEN_VAR_SORTED", ""))))
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--ks", default="31,40")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_var_seen.md"))
    ap.add_argument("--child", type=int, default=0, help="(internal) build once with this k and print the result")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reads)
    rows = []
    for k in (int(x) for x in a.ks.split(",")):
        for rep in range(-1, a.reps):                  # (rep -1: one child per k whose result is dropped -- the first one runs cold)
            for switch in ("1", "0") if rep >= 0 else ("1",):
                env = dict(os.environ, KATOME_SEEN_VAR_SORTED=switch)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), "--reads", str(a.reads)], env=env,
                                     capture_output=True, text=True, timeout=900)
                if out.returncode != 0:                # (a child that failed ends the run: nothing more is started on the card)
                    sys.stderr.write(out.stderr[-3000:])
                    return 1
                r = json.loads([line for line in out.stdout.splitlines() if line.startswith("RESULT ")][0][7:])
                if rep < 0:
                    continue
                r["rep"] = rep
                rows.append(r)
                print("k=%d rep %d sorted=%s: %.1f ms, %d edges, tile slots %d, k-mer slots %d" %
                      (k, rep, switch, r["wall_ms"], r["n_edges"], r["counts"]["tile_slots"], r["counts"]["kmer_slots"]), flush=True)
    lines = ["# First-seen builds of trimmed reads: levels by sorting against the tables", "",
             "`tools/bench_var_seen.py --reads %d --ks %s --reps %d`: c3's synthetic reads trimmed to 100..150 bases, first-seen order, both"
             % (a.reads, a.ks, a.reps),
             "strands, one GPU; every row one build in a fresh process, the two settings alternated. Times in ms.", ""]
    for k in sorted({r["k"] for r in rows}):
        mine = [r for r in rows if r["k"] == k]
        on, off = [r for r in mine if r["sorted"] == "1"], [r for r in mine if r["sorted"] == "0"]
        same = len({r["digest"] for r in mine}) == 1
        lines += ["## k = %d (span %d, %d edges; arrays of all runs %s)" % (k, mine[0]["span"], mine[0]["n_edges"], "equal" if same else "DIFFER"), "",
                  "| `KATOME_SEEN_VAR_SORTED` | wall per run | min | max | tile slots | k-mer slots |", "|---|---|---|---|---|---|"]
        for name, rs in (("1 (by sorting)", on), ("0 (tables)", off)):
            ws = [r["wall_ms"] for r in rs]
            lines.append("| %s | %s | %.1f | %.1f | %d | %d |" % (name, ", ".join("%.1f" % x for x in ws), min(ws), max(ws),
                                                              rs[0]["counts"]["tile_slots"], rs[0]["counts"]["kmer_slots"]))
        w_on, w_off = [r["wall_ms"] for r in on], [r["wall_ms"] for r in off]
        gain, spread = min(w_off) - max(w_on), max(max(w_on) - min(w_on), max(w_off) - min(w_off))
        lines += ["", "Slowest sorted run against the fastest table run: %+.1f ms; spread of the runs of one setting: %.1f ms -> %s." %
                  (-gain, spread, "faster by more than the spread" if gain > spread else "NOT faster by more than the spread"), "",
                  "| phase | by sorting (median) | tables (median) |", "|---|---|---|"]
        med = lambda rs, ph: sorted(r["phases"].get(ph, 0.0) for r in rs)[len(rs) // 2]
        for ph in sorted({p for r in mine for p in r["phases"]}):
            lines.append("| %s | %.1f | %.1f |" % (ph, med(on, ph), med(off, ph)))
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
