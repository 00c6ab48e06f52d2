"""Times the strand-unique assembly (katome_dev_collapse_unique, katome_dev_unique_contigs_arrays): the named text writer beside
text_write_kernel on the full text in the same run and beside a plain copy of the same bytes, the contig mirrors' parts beside the path
mirrors of katome_dev_collapse_gfa_strands, and the selection:
python tools/bench_unique.py [--reads 2000000] [--pieces 50000000] [--runs 3]   -> one JSON line

The two inputs of tools/bench_gfa_strand_paths.py:
  * an assembly: a by-key build of C3's first --reads reads (150 bp, k = 31, both strands), no stage; every run calls collapse("fasta")
    ("k:text_write_kernel" on the full text), collapse_unique("fasta") ("k:text_write_named_kernel", "k:unique_contigs selection" and
    the "k:mirror_*" entries on contigs) and collapse_gfa(merge_strands=True) (the "k:mirror_*" entries on paths), one after the other,
    so the runs alternate them; each text beside hipMemcpyAsync device to device of as many bytes;
  * a synthetic walk of --pieces pieces in contigs of 25 pieces on average over 2^20 labels of 40 bases, twin(i) = i ^ 1, the second
    half of the list the first half walked from its other end on the other strand: every contig is mirrored and half are dropped;
    through katome_dev_unique_contigs_arrays (KATOME_UNIQUE_TRACE=1 prints the kernels' times), and in the same run the full text of
    the same pieces through katome_dev_pieces_text (KATOME_TEXT_TRACE=1: "k:text_write_kernel").
What it prints: per quantity the median and the spread (min, max) over the runs; each writer's GB/s and its rate over the copy's."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["KATOME_UNIQUE_TRACE"] = "1"
os.environ["KATOME_TEXT_TRACE"] = "1"
import torch  # noqa: E402

from katome_amd import device as kd  # noqa: E402
from katome_amd.workloads import WORKLOADS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--pieces", type=int, default=50_000_000)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
MIRROR = {"k:mirror_sig_kernel": "mirror_sig_ms", "k:mirror signature sort": "mirror_sort_ms", "k:mirror_search_kernel": "mirror_search_ms",
          "k:mirror_verify_kernel": "mirror_verify_ms"}
NAMED, SELECT = "k:text_write_named_kernel", "k:unique_contigs selection"


def copy_ms(src, n):
    dst = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n, 3, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    e1.record()
    torch.cuda.synchronize()
    assert rc == 0
    return e0.elapsed_time(e1)


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


med = statistics.median
gbps = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9
summary = lambda v: {"median": med(v), "min": min(v), "max": max(v)}


def finish(d, runs):
    for n, v in runs.items():
        d[n] = summary(v)
    d["named_write_GBps"] = gbps(d["unique_bytes"], d["named_write_ms"]["median"])
    d["named_write_rate_over_copy"] = d["named_copy_ms"]["median"] / d["named_write_ms"]["median"]
    if "full_write_ms" in d:
        d["full_write_GBps"] = gbps(d["full_bytes"], d["full_write_ms"]["median"])
        d["full_write_rate_over_copy"] = d["full_copy_ms"]["median"] / d["full_write_ms"]["median"]
    d["contig_mirror_ms"] = sum(d["contig_" + n]["median"] for n in MIRROR.values())


out = {}

# ---- an assembly ---------------------------------------------------------------------------------------------------------------
w = WORKLOADS["c3"].scaled(args.reads)
packed, skip = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, 0, device=0)
b = kd.Builder(w.k, True, table_slots_hint=int(w.expected_distinct_canonical() * 2.2))
step = 4 << 20
for r0 in range(0, w.reads, step):
    b.count_reads(packed, min(step, w.reads - r0), w.read_len, None, first_read=r0)
dg = b.finalize()
out.update(reads=w.reads, k=w.k, genome_len=w.genome_len, edges=dg.n_edges, nodes=dg.n_nodes)
del dg, packed, skip
b.profile(True)
names = (["full_write_ms", "full_copy_ms", "named_write_ms", "named_copy_ms", "select_ms"] + ["contig_" + n for n in MIRROR.values()] + ["contig_mirror_rounds"] +
         ["path_" + n for n in MIRROR.values()])
runs = {n: [] for n in names}
for run in range(args.runs + 1):                # (run 0: warm-up)
    torch.cuda.synchronize()
    b.profile_read()
    a = b.collapse("fasta")
    prof = b.profile_read()
    vals = [prof["k:text_write_kernel"][0], copy_ms(a.text, a.text_bytes)]
    out.update(contigs=a.n_contigs, pieces=a.n_pieces, full_bytes=a.text_bytes)
    del a
    u = b.collapse_unique("fasta")
    prof = b.profile_read()
    vals += [prof[NAMED][0], copy_ms(u.text, u.text_bytes), prof[SELECT][0]]
    vals += [prof[k][0] if k in prof else 0.0 for k in MIRROR] + [prof["k:mirror_verify_kernel"][1] if "k:mirror_verify_kernel" in prof else 0]
    out.update(kept=u.n_kept, unique_bytes=u.text_bytes, mirrored=u.n_mirrored, self_mirror=u.n_self_mirror, unique_phase_ms=prof["unique_contigs"][0])
    del u
    g = b.collapse_gfa(merge_strands=True)
    prof = b.profile_read()
    vals += [prof[k][0] if k in prof else 0.0 for k in MIRROR]
    out.update(paths=g.n_paths, paths_mirrored=g.n_mirrored)
    del g
    if run:
        for n, v in zip(names, vals):
            runs[n].append(v)
finish(out, runs)
b.close()

# ---- a synthetic walk ----------------------------------------------------------------------------------------------------------
n_labels, P, k, bases = 1 << 20, args.pieces // 2 * 2, 31, 40
gen = torch.Generator(device="cuda").manual_seed(1)
stride = 1 + bases // 4                           # the pad byte (0: 40 bases fill 10 bytes) and the packed bases
labels = torch.randint(0, 256, (n_labels * stride + 16,), dtype=torch.uint8, device="cuda", generator=gen)
labels[torch.arange(n_labels, device="cuda") * stride] = 0
label_off = torch.arange(n_labels + 1, dtype=torch.int64, device="cuda") * stride
twin = torch.arange(n_labels, dtype=torch.int64, device="cuda") ^ 1
half = P // 2
ids = torch.randint(0, n_labels, (half,), device="cuda", generator=gen)
whole = torch.rand(half, device="cuda", generator=gen) < 0.04
whole[0] = True
last = torch.cat([whole[1:], torch.ones(1, dtype=torch.bool, device="cuda")])      # the pieces that end a contig begin its mirror
ids = torch.cat([ids, ids.flip(0) ^ 1])
whole = torch.cat([whole, last.flip(0)])
pieces = (ids | (whole.to(torch.int64) << 31)).to(torch.int32)      # (bit 31 set: the int32 wraps to the u32 the library reads)
del ids, whole, last
names = ["full_write_ms", "full_copy_ms", "named_write_ms", "named_copy_ms", "select_ms"] + ["contig_" + n for n in MIRROR.values()] + ["contig_mirror_rounds"]
runs = {n: [] for n in names}
syn = {}
for run in range(args.runs + 1):
    (c_off, c_len, text, n_bytes), err = traced(lambda: kd.pieces_text(labels, label_off, pieces, k, "fasta"))
    m = re.search(r"k:text_write_kernel ([0-9.]+) ms, (\d+) bytes", err)
    assert m and int(m.group(2)) == n_bytes, err
    full = [float(m.group(1)), copy_ms(text, n_bytes)]
    syn.update(full_bytes=n_bytes)
    del c_off, c_len, text
    u, err = traced(lambda: kd.unique_contigs_arrays(labels, label_off, twin, pieces, k, "fasta"))
    got = {}
    for name, ms in re.findall(r"\[katome_dev_unique_contigs_arrays\] (k:[^0-9]*?) ([0-9.]+) ms", err):
        got.setdefault(name, []).append(float(ms))
    assert NAMED in got and SELECT in got, err
    vals = full + [sum(got[NAMED]), copy_ms(u.text, u.text_bytes), sum(got[SELECT])]
    vals += [sum(got.get(k, [0.0])) for k in MIRROR] + [len(got.get("k:mirror_verify_kernel", []))]
    syn.update(pieces=P, labels=n_labels, contigs=u.n_contigs, kept=u.n_kept, unique_bytes=u.text_bytes, mirrored=u.n_mirrored, self_mirror=u.n_self_mirror)
    del u
    if run:
        for n, v in zip(names, vals):
            runs[n].append(v)
finish(syn, runs)
out["synthetic"] = syn
print(json.dumps(out), flush=True)
