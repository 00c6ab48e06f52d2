"""The two list-fed levels' records are no longer written before their first partition pass: that pass cuts them out of the list
(radix.hip, ListSource) and a count-only kernel makes its per-tile digit counts (table.hip, list_digit_counts_kernel).  The records
after the pass, the counts and whole builds must be byte for byte what the written records give (KATOME_FUSED_RECORDS=0).  The switch
is read once, so every setting of a whole build runs in a child process of its own, each under a time limit; a child that ends any
other way than with status 0 fails its test, which then starts nothing more."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, tile_bases, k, span, stride, rc, rep): the mid level of k = 31 (two-word sub-tiles by hash, 2048-record sort tiles, with the
# next pass's digit bytes), its k-mer level with both strands and with one, and one-word tiles into k-mers at k = 13
_FORMS = [("mid_2_2", 60, 36, 5, 6, 1, 0), ("kmers_2_1_rc", 36, 31, 6, 1, 1, 1), ("kmers_2_1_one_strand", 36, 31, 6, 1, 0, 1),
          ("kmers_1_1_rc", 18, 13, 6, 1, 1, 1), ("kmers_1_1_one_strand", 18, 13, 6, 1, 0, 1)]


def _entry_counts(span, sort_tile):
    """list entries to run: none, one, the counts whose records lie next to one sort tile on both sides (with the tile itself where
    span divides it, and one tile less one record where that is a whole entry), 3 tiles + 1, and about 40 and 70 tiles -- the tile
    numbering changes at 64.  Neither 2048 nor 4096 is a multiple of 5 or 6: entries straddle every tile boundary"""
    out = {0, 1, (sort_tile - 1) // span, sort_tile // span, -(-sort_tile // span), -(-(3 * sort_tile + 1) // span),
           40 * sort_tile // span + 1, 70 * sort_tile // span + 1}
    return sorted(out)


_PRIMITIVE_SCRIPT = r"""
import sys, hashlib, ctypes as C, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from katome_amd import _lib, device as kd
forms = eval(sys.argv[2]); counts = eval(sys.argv[3])
L = _lib.lib()
rng = np.random.default_rng(15)
def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:24]
for (name, tile_bases, k, span, stride, rc, rep) in forms:
    nwt = 1 if tile_bases <= 32 else 2
    nwk = 1 if k <= 32 else 2
    sort_tile = 4096 if nwk == 1 else 2048
    for n_tiles in counts[name]:
        words = rng.integers(0, 1 << 63, size=(max(n_tiles, 1), nwt), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(max(n_tiles, 1), nwt), dtype=np.uint64)
        top_bits = 2 * tile_bases - 64 * (nwt - 1)
        if top_bits < 64:
            words[:, 0] &= np.uint64((1 << top_bits) - 1)
        cnt = rng.integers(1, 1 << 16, size=max(n_tiles, 1), dtype=np.uint32)
        d_tiles = torch.from_numpy(words.view(np.int64).reshape(-1).copy()).cuda()
        d_cnt = torch.from_numpy(cnt.view(np.int32).copy()).cuda()
        n = n_tiles * span
        n_sort = (n + sort_tile - 1) // sort_tile
        for fused in (1, 0):
            keys = torch.zeros(max(n, 1) * nwk, dtype=torch.int64, device="cuda")
            wts = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
            dc = torch.zeros(max(n_sort, 1) * 256, dtype=torch.int32, device="cuda")
            st = L.katome_dev_list_first_pass(0, kd._ptr(d_tiles), kd._ptr(d_cnt), n_tiles, tile_bases, k, span, stride, rc, rep, fused,
                                              kd._ptr(keys), kd._ptr(wts), kd._ptr(dc), kd._stream())
            assert st == 0, (name, n_tiles, fused, st, _lib.last_error())
            torch.cuda.synchronize()
            assert int(dc.sum().item()) == n, (name, n_tiles, fused)
            print("FP", name, n_tiles, n, "fused" if fused else "written", sha(keys), sha(wts), sha(dc), int(wts.to(torch.int64).sum().item()), flush=True)
"""

_BUILD_SCRIPT = r"""
import sys, hashlib, random, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii, int_to_kmer
from oracle import oracle as o
from katome_amd import device as kd

def digest(name, reads, k, rc, min_weight=0, oracle=False):
    print("BUILD " + name, file=sys.stderr, flush=True)
    L = reads.shape[1]
    has_n = (reads == ord("N")).any(axis=1)
    skip = None
    packed_from = reads
    if has_n.any():                                   # a read with an N is skipped whole; its N's are packed as A's
        packed_from = reads.copy(); packed_from[packed_from == ord("N")] = ord("A")
        skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    packed = torch.from_numpy(pack_reads_ascii(packed_from).reshape(-1).copy()).cuda()
    b = kd.Builder(k, rc)
    if min_weight:
        b.remove_weak_edges(min_weight)
    b.count_reads(packed, len(reads), L, skip, first_read=0)
    dg = b.finalize()
    arrays = [t.cpu().numpy() for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label)]
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    print("FR", name, dg.n_nodes, dg.n_edges, h.hexdigest(), flush=True)
    if oracle:                                        # (one-word k-mers)
        ref = o.build_ascii(reads, k, rc)
        got = sorted(zip((int_to_kmer(int(v), k) for v in arrays[0].reshape(-1).view(np.uint64)), (int(w) for w in arrays[1])))
        assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges), (name, dg.n_nodes, dg.n_edges, ref.n_nodes, ref.n_edges)
        assert got == ref.multiset(), name
        print("ORACLE", name, "equal", flush=True)
    del dg
    b.close()

for k in (11, 13, 21, 31):                                            # odd k, both strands
    digest("k%d" % k, o.synth_reads(k, 3000, 150, 30000, 3e-3, 0), k, True, oracle=(k == 31))
digest("one_strand_k31", o.synth_reads(3, 3000, 150, 30000, 3e-3, 0), 31, False)
digest("min_weight", o.synth_reads(5, 3000, 150, 20000, 3e-3, 0), 31, True, 3)
digest("even_k_both_strands", o.synth_reads(13, 3000, 150, 30000, 3e-3, 0), 20, True)       # (no ordered count: hash digits at the k-mer level)
digest("two_word_k40", o.synth_reads(11, 3000, 150, 30000, 3e-3, 0), 40, True)              # (three-word tiles)
digest("left_over_windows", o.synth_reads(6, 3000, 101, 30000, 3e-3, 0), 31, True)          # (101 bp: windows that are not whole tiles)
digest("reads_with_n", o.synth_reads(9, 3000, 150, 30000, 3e-3, 5), 31, True)
rng = random.Random(7)
lowc = ["A" * 37 + "".join(rng.choice("ACGT") for _ in range(23)) for _ in range(3000)]
digest("low_complexity", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 31, True)
rng = random.Random(8)
lowc = ["A" * 12 + "".join(rng.choice("ACGT") for _ in range(88)) for _ in range(3000)]
digest("low_complexity_short_run", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 21, True)
digest("five_reads", o.synth_reads(16, 5, 150, 30000, 3e-3, 0), 31, True)                   # (every level has less than one sort tile)
"""

_N_BUILDS = 13
_MADE = "made by their first partition pass"
_WRITTEN = "written ("
_LEFT_OVER = "written (left-over windows go behind them)"
_SWITCHED_OFF = "written (KATOME_FUSED_RECORDS=0)"


def _run(script, args, timeout, **env_extra):
    env = dict(os.environ, KATOME_LC_TRACE="1", **env_extra)
    out = subprocess.run([sys.executable, "-c", script, ROOT] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    return out


def _rows(out, tag):
    return [line for line in out.stdout.splitlines() if line.startswith(tag + " ")]


def _by_build(out):
    parts = out.stderr.split("BUILD ")[1:]
    return {p.split("\n", 1)[0].strip(): p for p in parts}


def test_first_pass_off_the_list_equals_the_pass_over_written_records():
    """every form and count through katome_dev_list_first_pass, both routes in one process: keys, weights and the per-tile digit
    counts (list_digit_counts_kernel against list_to_records_hist_kernel) byte for byte"""
    counts = {f[0]: _entry_counts(f[3], 4096 if f[2] <= 32 else 2048) for f in _FORMS}
    out = _run(_PRIMITIVE_SCRIPT, [repr(_FORMS), repr(counts)], 300)
    rows = _rows(out, "FP")
    assert len(rows) == 2 * sum(len(c) for c in counts.values())
    fused = [r.split() for r in rows if r.split()[4] == "fused"]
    written = [r.split() for r in rows if r.split()[4] == "written"]
    assert len(fused) == len(written)
    for a, b in zip(fused, written):
        assert a[:4] == b[:4] and a[5:] == b[5:], (a, b)
    # (and the two routes were two routes)
    assert out.stderr.count(_MADE) == sum(1 for c in counts.values() for n in c if n)
    # the tile numbering was taken both ways
    tiles = [int(r[3]) // (4096 if "kmers" in r[1] else 2048) for r in fused]
    assert any(3 < t < 64 for t in tiles) and any(t >= 64 for t in tiles)


def test_builds_equal_with_records_written_first():
    """whole builds, default against KATOME_FUSED_RECORDS=0, with the ordered count and (KATOME_EDGE_HALF_SORT=0) without it; one
    build against the oracle; the trace says which way every list-fed level's records were made"""
    base = dict(KATOME_SORTED_COUNT="2")          # (the k-mer level counted by sorting however small the input)
    new = _run(_BUILD_SCRIPT, [], 600, **base)
    rows = _rows(new, "FR")
    assert len(rows) == _N_BUILDS
    assert _rows(new, "ORACLE") == ["ORACLE k31 equal"]
    old = _run(_BUILD_SCRIPT, [], 600, **base, KATOME_FUSED_RECORDS="0")
    assert _rows(old, "FR") == rows
    new_full = _run(_BUILD_SCRIPT, [], 600, **base, KATOME_EDGE_HALF_SORT="0")
    assert _rows(new_full, "FR") == rows
    old_full = _run(_BUILD_SCRIPT, [], 600, **base, KATOME_EDGE_HALF_SORT="0", KATOME_FUSED_RECORDS="0")
    assert _rows(old_full, "FR") == rows
    for run in (old, old_full):
        assert _MADE not in run.stderr
        assert run.stderr.count(_SWITCHED_OFF) == run.stderr.count("[records] ") > 0
    traces = _by_build(new)
    assert len(traces) == _N_BUILDS
    # both levels of k = 31 at 150 bp (big tiles of 30 windows, mid tiles of 6, nothing left over) leave their records to the first pass,
    # with both strands and with one ...
    for name in ("k31", "one_strand_k31", "min_weight", "reads_with_n", "five_reads"):
        assert traces[name].count(_MADE) == 2 and _WRITTEN not in traces[name], (name, traces[name][-1500:])
    # ... k = 11 (tiles of 28 windows, nothing left over; its mid tiles are one-word records ordered by hash: written) its k-mers' ...
    assert traces["k11"].count(_MADE) == 1, traces["k11"][-1500:]
    # ... 101-bp reads leave a window over per read, which goes behind the k-mer records: those are written, and say so ...
    assert traces["left_over_windows"].count(_LEFT_OVER) == 1 and _MADE not in traces["left_over_windows"], traces["left_over_windows"][-1500:]
    # ... and so do k = 13, 20 and 21 at 150 bp; two-word k-mers are written as before
    for name in ("k13", "k21", "even_k_both_strands"):
        assert _LEFT_OVER in traces[name], (name, traces[name][-1500:])
    assert _MADE not in traces["two_word_k40"]
    # a group that fills its table sends the ordered count back after the passes: the records must be there for the hash groups
    assert traces["low_complexity"].count(_MADE) == 2, traces["low_complexity"][-1500:]
