"""Three passes the result never needed, each behind a switch that is read once (so every setting runs in a process of its own):
a level's list trimmed where it lies instead of copied (KATOME_TRIM_IN_PLACE), the source run heads counted by the merge that
writes the edges (KATOME_MERGE_HEADS) and the labels written by the pass that writes the source ids (KATOME_LABELS_IN_IDS).
Every setting, and every merge route that supplies no head counts, must give byte for byte the same arrays."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SMALL_SCRIPT = r"""
import sys, os, hashlib, random, tempfile, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes

def show(name, n_nodes, n_edges, arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    print("FI", name, n_nodes, n_edges, h.hexdigest(), flush=True)

def digest(name, reads, k, rc, min_weight=0, edges_first=False, first_seen=False):
    print("BUILD " + name, file=sys.stderr, flush=True)
    L = reads.shape[1]
    has_n = (reads == ord("N")).any(axis=1)
    skip = None
    if has_n.any():                                   # a read with an N is skipped whole; its N's are packed as A's
        reads = reads.copy(); reads[reads == ord("N")] = ord("A")
        skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, rc, first_seen_order=first_seen)
    if min_weight:
        b.remove_weak_edges(min_weight)
    b.count_reads(packed, len(reads), L, skip, first_read=0)
    if edges_first:
        ek, ew = b.edges()
        assert ek.shape[0] == ew.shape[0]
        del ek, ew
    dg = b.finalize()
    if first_seen:
        del dg
        dg, _ = b.remove_dead_paths()
    show(name, dg.n_nodes, dg.n_edges, [t.cpu().numpy() for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label)])
    del dg
    b.close()

for k in (11, 13, 17, 21, 25, 31):                                    # odd k, both strands
    digest("k%d" % k, o.synth_reads(k, 4000, 150, 30000, 3e-3, 0), k, True)
digest("one_strand_k31", o.synth_reads(3, 3000, 150, 30000, 3e-3, 0), 31, False)
digest("min_weight", o.synth_reads(5, 4000, 150, 20000, 3e-3, 0), 31, True, 3)
digest("left_over_windows", o.synth_reads(6, 4000, 101, 30000, 3e-3, 0), 31, True)      # (101 bp: windows that are not whole tiles)
rng = random.Random(7)
lowc = ["A" * 37 + "".join(rng.choice("ACGT") for _ in range(23)) for _ in range(3000)]
digest("low_complexity", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 31, True)
rng = random.Random(8)
lowc = ["A" * 12 + "".join(rng.choice("ACGT") for _ in range(88)) for _ in range(3000)]
digest("low_complexity_short_run", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 21, True)
digest("reads_with_n", o.synth_reads(9, 4000, 150, 30000, 3e-3, 5), 31, True)
digest("edges_before_finalize", o.synth_reads(10, 4000, 150, 30000, 3e-3, 0), 27, True, edges_first=True)
digest("two_word_k40", o.synth_reads(11, 3000, 150, 30000, 3e-3, 0), 40, True)          # (two-word keys: no ordered count, so no merge)
digest("two_word_k63", o.synth_reads(12, 2000, 150, 30000, 3e-3, 0), 63, False)
digest("even_k_both_strands", o.synth_reads(13, 4000, 150, 30000, 3e-3, 0), 20, True)  # (palindromes: the full edge sort)
digest("first_seen_dead_paths", o.synth_reads(14, 3000, 150, 30000, 3e-3, 0), 31, True, first_seen=True)

# the host entry points: packed reads, then BFCounter lines (their edges are installed as listed: no merge made them)
print("BUILD host_packed", file=sys.stderr, flush=True)
reads = o.synth_reads(15, 3000, 150, 30000, 3e-3, 0)
g, _ = GpuGraph.create_from_packed(pack_reads_ascii(reads).reshape(-1).copy(), len(reads), 150, reverse_complement=True, k=31)
show("host_packed", g.n_nodes, g.n_edges, [g.edge_key, g.edge_weight, g.edge_src, g.edge_dst, g.node_key, g.edge_label])
ref = o.build_ascii(reads, 31, True)
print("BUILD host_bfc", file=sys.stderr, flush=True)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "kmers.bfc")
    open(path, "w").write("".join("%s\t%d\n" % (km, w) for km, w in sorted(ref.multiset())[::2]))
    set_global_k_sizes(31)
    g, _ = GpuGraph.create([path], InputFileType.BFCounter, True, 0)
    show("host_bfc", g.n_nodes, g.n_edges, [g.edge_key, g.edge_weight, g.edge_src, g.edge_dst, g.node_key, g.edge_label])
"""

_BIG_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from katome_amd import device as kd
from katome_amd.workloads import WORKLOADS
wl = WORKLOADS[sys.argv[2]]
if len(sys.argv) > 3:
    wl = wl.scaled(int(sys.argv[3]))
packed, _ = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, 0)
b = kd.Builder(wl.k, True, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2))
for r0 in range(0, wl.reads, 4 << 20):
    b.count_reads(packed, min(4 << 20, wl.reads - r0), wl.read_len, None, first_read=r0)
del packed
dg = b.finalize()
sums = []
for a in (dg.edge_key.reshape(-1), dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key.reshape(-1), dg.edge_label.reshape(-1)):
    total, n = 0, a.numel()
    for i in range(0, n, 1 << 27):                     # sum of a[i] * (2 i + 1) mod 2^64: order and value of every word
        z = min(n, i + (1 << 27))
        w = torch.arange(i, z, device=a.device, dtype=torch.int64) * 2 + 1
        total = (total + int((a[i:z].to(torch.int64) * w).sum().item())) & ((1 << 64) - 1)
    sums.append(total)
print("BIG", dg.n_nodes, dg.n_edges, int(dg.edge_weight.to(torch.int64).sum().item()), *sums, flush=True)
"""

_HEADS = "[node ids] heads from the merge"
_LABELS = "[node ids] labels written with the source ids"
_TRIMMED = "[levels] list trimmed in place"
_GROUPED = "ordered per group in the merge"          # (lds_count.hip half_sort_finish: the edges leave group_merge_kernel)
_ALL_OFF = dict(KATOME_TRIM_IN_PLACE="0", KATOME_MERGE_HEADS="0", KATOME_LABELS_IN_IDS="0")
# the builds whose edges leave group_merge_kernel (one-word k-mers of odd k, both strands, default numbering) ...
_MERGED = ["k11", "k13", "k17", "k21", "k25", "k31", "min_weight", "left_over_windows", "reads_with_n", "edges_before_finalize", "host_packed"]
# ... those that may (k-mers crowding a few key prefixes can fill a group's table: the count then goes by hash groups, without a merge) ...
_LOW_COMPLEXITY = ["low_complexity", "low_complexity_short_run"]
# ... and those that must not be handed head counts: no S2, two-word keys, the full edge sort, first-seen order, listed edges
_NOT_MERGED = ["one_strand_k31", "two_word_k40", "two_word_k63", "even_k_both_strands", "first_seen_dead_paths", "host_bfc"]
_N_BUILDS = len(_MERGED) + len(_LOW_COMPLEXITY) + len(_NOT_MERGED)


def _run(script, args, timeout, **env_extra):
    env = dict(os.environ, KATOME_LC_TRACE="1", **env_extra)
    out = subprocess.run([sys.executable, "-c", script, ROOT] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def _rows(out, tag):
    return [line for line in out.stdout.splitlines() if line.startswith(tag + " ")]


def _by_build(out):
    """the trace lines of every build of _SMALL_SCRIPT: {name: text}"""
    parts = out.stderr.split("BUILD ")[1:]
    return {p.split("\n", 1)[0].strip(): p for p in parts}


def test_small_builds_equal_every_setting():
    """odd k from 11 to 31, one strand, min_weight > 0, 101-bp reads, low-complexity input, reads with N, edges() before finalize(),
    two-word k-mers, even k, first-seen order with remove_dead_paths and the host entry points: the same arrays with every switch on,
    each off alone, all off, and on the merge routes that count no heads"""
    base = dict(KATOME_SORTED_COUNT="2")          # (the k-mer level counted by sorting however small the input)
    new = _run(_SMALL_SCRIPT, [], 900, **base)
    rows = _rows(new, "FI")
    assert len(rows) == _N_BUILDS
    runs = {"new": new}
    for name, extra in (("no_trim", dict(KATOME_TRIM_IN_PLACE="0")), ("no_heads", dict(KATOME_MERGE_HEADS="0")),
                        ("no_labels", dict(KATOME_LABELS_IN_IDS="0")), ("all_off", _ALL_OFF),
                        ("s2_sort", dict(KATOME_S2_GROUP_SORT="0")), ("capped", dict(KATOME_S2_GROUP_CAP="1")),
                        ("full_sort", dict(KATOME_EDGE_HALF_SORT="0"))):
        runs[name] = _run(_SMALL_SCRIPT, [], 900, **base, **extra)
        assert _rows(runs[name], "FI") == rows, name
    # the new paths ran where they should, and only there: head counts exactly where group_merge_kernel made the edges
    traces = _by_build(new)
    assert sorted(traces) == sorted(_MERGED + _LOW_COMPLEXITY + _NOT_MERGED)
    for name, text in traces.items():
        assert text.count(_HEADS) == text.count(_GROUPED), (name, text[-1500:])
        assert text.count(_GROUPED) == (1 if name in _MERGED else 0) or name in _LOW_COMPLEXITY, (name, text[-1500:])
        # (first-seen order renumbers the edges first: dev_labels afterwards)
        assert text.count(_LABELS) == (0 if name == "first_seen_dead_paths" else 1), (name, text[-1500:])
    for name in ("no_heads", "all_off", "s2_sort", "capped", "full_sort"):
        assert _HEADS not in runs[name].stderr, name
    for name in ("no_trim", "no_labels"):
        assert runs[name].stderr.count(_HEADS) == new.stderr.count(_HEADS), name
    for name in ("no_trim", "no_heads", "s2_sort", "capped", "full_sort"):
        assert runs[name].stderr.count(_LABELS) == _N_BUILDS - 1, name
    for name in ("no_labels", "all_off"):
        assert _LABELS not in runs[name].stderr, name


def test_c2_equals_all_switches_off():
    """C2 in full: weights, order and position-weighted checksums of every array as with the three switches off"""
    new = _run(_BIG_SCRIPT, ["c2"], 1200)
    old = _run(_BIG_SCRIPT, ["c2"], 1200, **_ALL_OFF)
    assert _rows(new, "BIG")[-1] == _rows(old, "BIG")[-1]
    assert _HEADS in new.stderr and _LABELS in new.stderr, new.stderr[-2000:]
    assert _HEADS not in old.stderr and _LABELS not in old.stderr and _TRIMMED not in old.stderr


def test_lists_of_a_gibibyte_are_trimmed_in_place():
    """a level's list is only worth trimming from 1 GiB (count_routes.hip shrink_to_fit): C3's coverage on 24 M reads, whose tile levels' key
    lists are 1.4-1.5 GiB for about a fifth of that used -- trimmed in place, the same checksums as copied"""
    new = _run(_BIG_SCRIPT, ["c3", "24000000"], 1200)
    old = _run(_BIG_SCRIPT, ["c3", "24000000"], 1200, **_ALL_OFF)
    assert _rows(new, "BIG")[-1] == _rows(old, "BIG")[-1]
    assert new.stderr.count(_TRIMMED) >= 2, new.stderr[-2000:]
    assert _HEADS in new.stderr and _LABELS in new.stderr
    assert _TRIMMED not in old.stderr
