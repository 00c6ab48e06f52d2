"""The partition passes' histograms without a second read of the keys: the kernel that places a record for a pass also leaves that
pass's digit, one byte, at the record's index (radix.hip radix_scatter_kernel with a next digit, lds_count.hip lds_count_ordered_kernel
for S2), and the pass counts its tiles from those bytes (digit_hist_kernel); the big tiles' first pass takes its counts from the
extraction that wrote the records (extract.hip extract_fixed_kernel, HIST).  The counts are the same numbers from another source,
so every array of every build must be byte for byte what the routes that use no partition pass at all give (both tile levels and
the k-mers counted in tables) and what the two-call boundary extract_tiles + insert_tiles gives; node and edge counts and the
weight sum are also the oracle's.
The switches are read once, so every setting runs in a process of its own."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import sys, hashlib, random, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd

which = sys.argv[2]
two_calls = len(sys.argv) > 3 and sys.argv[3] == "two_calls"

def show(name, dg, extra=""):
    h = hashlib.sha256()
    for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
        h.update(t.cpu().numpy().tobytes())
    print("DS", name, dg.n_nodes, dg.n_edges, h.hexdigest(), extra, flush=True)

def random_reads(seed, n, L):
    rng = np.random.RandomState(seed)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size=(n, L))]

def pack(reads):
    has_n = (reads == ord("N")).any(axis=1)
    skip = None
    if has_n.any():                                   # a read with an N is skipped whole; its N's are packed as A's
        reads = reads.copy(); reads[reads == ord("N")] = ord("A")
        skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    return torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda(), skip, has_n

def batches(name, reads, k, rc, sizes, min_weight=0, check=True, also=None):
    # the reads counted in batches of the given sizes (the last one takes what is left): count_tiles, or extract_tiles + insert_tiles
    print("BUILD " + name, file=sys.stderr, flush=True)
    L = reads.shape[1]
    packed, skip_all, has_n = pack(reads)
    b = kd.Builder(k, rc)
    if min_weight:
        b.remove_weak_edges(min_weight)
    span, tiles, rest = b.tile_plan(L)
    assert span > 1
    r0 = 0
    for i in range(len(sizes) + 1):
        n = sizes[i] if i < len(sizes) else len(reads) - r0
        if n <= 0:
            break
        skip = skip_all if has_n[r0:r0 + n].any() else None          # (a batch of clean reads comes without a skip array)
        if two_calls:
            b.insert_tiles(b.extract_tiles(packed, n, L, span, skip, first_read=r0), span)
        else:
            b.count_tiles(packed, n, L, span, skip, first_read=r0)
        if rest:
            b.insert(b.extract_remainder(packed, n, L, span, skip, first_read=r0))
        r0 += n
    assert r0 == len(reads)
    if also is not None:                              # one more read of another length whose tiles the build has already
        p2, _, _ = pack(also)
        b.count_tiles(p2, len(also), also.shape[1], span, None)
        b.insert(b.extract_remainder(p2, len(also), also.shape[1], span, None))
    dg = b.finalize()
    ok = ""
    if check and also is None:
        ref = o.build_ascii(reads, k, rc, remove_weak_edges=min_weight) if min_weight else o.build_ascii(reads, k, rc)
        assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges), (name, dg.n_nodes, dg.n_edges, ref.n_nodes, ref.n_edges)
        assert int(dg.edge_weight.sum().item()) == int(ref.edge_weight.astype("uint64").sum()), name
        ok = "oracle"
    show(name, dg, ok)
    del dg
    b.close()

if which == "tiles":
    # count_tiles batches: 4 tile records a read (150 bp, k = 31), 2048 records a sort tile = 512 reads
    reads = o.synth_reads(21, 6000, 150, 40000, 3e-3, 0)
    batches("whole_sort_tiles", reads, 31, True, [1024, 2048, 512, 1536])                # every batch starts on a tile boundary
    batches("first_batch_64_odd", reads, 31, True, [64 * 7, 2048, 1024])                 # ... the later ones off it
    batches("smaller_than_a_tile", reads[:300], 31, True, [300])
    batches("tile_and_a_bit", reads[:513], 31, True, [512, 1])
    withn = o.synth_reads(22, 6000, 150, 40000, 3e-3, 7)                                 # reads with N: skipped between clean ones
    assert (withn == ord("N")).any()
    batches("skipped_reads", withn, 31, True, [1024, 2048, 1024])
    clean_then_n = np.concatenate([reads[:2048], withn[:1024], reads[2048:4096]])
    batches("skipped_reads_between_clean_batches", clean_then_n, 31, True, [2048, 1024, 2048])
    # (room for 16 batches like the first to begin with: the kept array and its counts grow)
    batches("more_batches_than_room", o.synth_reads(29, 12000, 150, 40000, 3e-3, 0), 31, True, [512] * 23)
    batches("more_batches_than_room_off_boundary", reads, 31, True, [64] + [256] * 20)
elif which == "levels":
    # 158-bp reads that share nothing: 128 windows a read in 4 tiles of span 32, mid tiles of span 4 -- 32 mid records and 128 k-mer
    # records a read.  A sort tile is 2048 two-word records (the mid level: 64 reads) and 4096 one-word ones (the k-mers: 32 reads).
    # The mid level's records come 8 to a big tile, so "a tile plus one" is a tile plus 8 there; the k-mer level gets its one
    # record more from a 159-bp read that repeats a read the build has and so adds one left-over window and no tile.
    for n in (31, 32, 33, 63, 64, 65):
        batches("distinct_reads_%d" % n, random_reads(30 + n, n, 158), 31, True, [n])
    r = random_reads(40, 32, 158)
    longer = np.concatenate([r[:1], np.frombuffer(b"C", dtype=np.uint8).reshape(1, 1)], axis=1)
    batches("distinct_reads_32_plus_one_window", r, 31, True, [32], also=longer)
elif which == "shapes":
    batches("r101", o.synth_reads(23, 5000, 101, 40000, 3e-3, 0), 31, True, [2000, 2000])     # left-over windows join the k-mer level
    batches("k40", o.synth_reads(24, 4000, 150, 40000, 3e-3, 0), 40, True, [1500, 1500])       # three-word tiles, two-word mid tiles and k-mers
    batches("k63", o.synth_reads(25, 3000, 150, 40000, 3e-3, 0), 63, True, [1000, 1000])
    batches("k63_one_strand", o.synth_reads(26, 3000, 150, 40000, 3e-3, 0), 63, False, [3000])
    batches("min_weight", o.synth_reads(27, 5000, 150, 20000, 3e-3, 0), 31, True, [2048], min_weight=3)
    batches("one_strand", o.synth_reads(28, 4000, 150, 40000, 3e-3, 0), 31, False, [2048])
    rng = random.Random(7)
    lowc = ["A" * 37 + "".join(rng.choice("ACGT") for _ in range(113)) for _ in range(3000)]
    batches("low_complexity", np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in lowc]), 31, True, [1024])
"""

_BY_HASH = re.compile(r"\[order\] by hash: (\d+) records of (\d) words, first pass counted from (its writer's counts|the keys), second from (the digit stream|the keys)")
_BY_KEY = re.compile(r"\[order\] by key: (\d+) records of 1 words, first pass counted from (its writer's counts|its writer's digits|the keys), second from (the digit stream|the keys)")
_SORTED = dict(KATOME_SORTED_COUNT="2")              # (every level counted by sorting however small the input)
_TABLES = dict(KATOME_SORTED_COUNT="0", KATOME_SORTED_TILES="0")      # (no level counted by sorting: no partition pass anywhere)


def _run(which, extra_args=(), **env_extra):
    env = dict(os.environ, KATOME_LC_TRACE="1", **env_extra)
    out = subprocess.run([sys.executable, "-c", _SCRIPT, ROOT, which] + list(extra_args), env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def _rows(out):
    rows = [line for line in out.stdout.splitlines() if line.startswith("DS ")]
    assert rows
    return rows


def _by_build(out):
    parts = out.stderr.split("BUILD ")[1:]
    return {p.split("\n", 1)[0].strip(): p for p in parts}


def test_count_tiles_batches():
    """batches that are whole sort tiles, a first batch of 64 x odd reads, skipped reads between clean batches, more batches than the
    kept array first has room for, a batch smaller than a sort tile: the same arrays as through extract_tiles + insert_tiles (which
    supplies no counts), as with KATOME_FUSED_HIST=0 and as with every level in tables; node and edge counts and the weight sum as the
    oracle's"""
    new = _run("tiles", **_SORTED)
    rows = _rows(new)
    assert len(rows) == 8 and all(r.endswith(" oracle") for r in rows)
    two_calls = _run("tiles", ["two_calls"], **_SORTED)
    assert _rows(two_calls) == rows
    assert _rows(_run("tiles", **_SORTED, KATOME_FUSED_HIST="0")) == rows
    tables = _run("tiles", **_TABLES)
    assert _rows(tables) == rows
    assert "[order]" not in tables.stderr
    # where the extraction's counts hold -- every batch written in place from a sort-tile boundary on -- the big tiles' first pass
    # takes them; everywhere else, and through the two-call boundary, it counts from the keys
    holds = dict(whole_sort_tiles=True, first_batch_64_odd=False, smaller_than_a_tile=True, tile_and_a_bit=True, skipped_reads=False,
                 skipped_reads_between_clean_batches=False, more_batches_than_room=True, more_batches_than_room_off_boundary=False)
    traces, traces2 = _by_build(new), _by_build(two_calls)
    assert sorted(traces) == sorted(holds)
    for name, text in traces.items():
        # the big tiles (two words, no weights), the mid tiles and the k-mers: each level's second pass reads the digit stream
        by_hash = _BY_HASH.findall(text)
        assert len(by_hash) == 2 and len(_BY_KEY.findall(text)) == 2, (name, text[-1500:])
        # records of two words take the second pass's counts from the digit stream; one-word records stay on the keys (radix.hip
        # digit_stream_pays: their balance came out level)
        assert [second for _, _, _, second in by_hash] == ["the digit stream"] * 2, (name, text[-1500:])
        assert [second for _, _, second in _BY_KEY.findall(text)] == ["the keys"] * 2, (name, text[-1500:])
        assert by_hash[0][1] == "2" and by_hash[0][2] == ("its writer's counts" if holds[name] else "the keys"), (name, text[-1500:])
        assert _BY_HASH.findall(traces2[name])[0][2] == "the keys", name
        if name.startswith("skipped"):
            # a batch with a skip array is not written in place and says nothing; no batch after it may be counted by the extraction
            said = re.findall(r"\[tiles\] batch of \d+ records at (\d+): (first-pass counts from the extraction|no counts)", text)
            first_skipped = {"skipped_reads": 0, "skipped_reads_between_clean_batches": 4 * 2048}[name]
            assert all(int(at) < first_skipped for at, what in said if what != "no counts"), (name, said)
            assert len(said) == (0 if name == "skipped_reads" else 1), (name, said)
        else:
            assert ("no counts" in text) == (not holds[name]), (name, text[-1500:])


def test_record_counts_around_a_sort_tile():
    """the mid level with 2016, 2048 and 2080 records (a sort tile of two-word records is 2048; the level's records come 8 to a big
    tile) and the k-mer level with 3968, 4096, 4097 and 4224 (a tile of one-word records is 4096)"""
    new = _run("levels", **_SORTED)
    rows = _rows(new)
    assert len(rows) == 7
    assert _rows(_run("levels", **_TABLES)) == rows
    traces = _by_build(new)
    mid = {name: [int(n) for n, nw, _, _ in _BY_HASH.findall(text)] for name, text in traces.items()}
    kmers = {name: [int(n) for n, _, _ in _BY_KEY.findall(text)][0] for name, text in traces.items()}
    for n in (31, 32, 33, 63, 64, 65):
        assert mid["distinct_reads_%d" % n] == [4 * n, 32 * n], mid            # (big tiles, then mid tiles)
        assert kmers["distinct_reads_%d" % n] == 128 * n, kmers
    assert kmers["distinct_reads_32_plus_one_window"] == 4097, kmers


def test_other_shapes_and_s2_routes():
    """101-bp reads (left-over windows join the k-mer level: no counts from the writer), k = 40
    and k = 63 (two- and three-word records), min_weight, one strand, low-complexity input that makes the ordered count fall back
    to the hash groups; S2 on its default route, sorted in full because of KATOME_S2_GROUP_CAP (the digits are ignored) and with
    KATOME_S2_GROUP_SORT=0"""
    new = _run("shapes", **_SORTED)
    rows = _rows(new)
    assert len(rows) == 7
    assert sum(r.endswith(" oracle") for r in rows) == 7
    for extra in (dict(KATOME_S2_GROUP_CAP="1"), dict(KATOME_S2_GROUP_SORT="0"), dict(KATOME_EDGE_HALF_SORT="0")):
        assert _rows(_run("shapes", **_SORTED, **extra)) == rows, extra
    assert _rows(_run("shapes", **_TABLES)) == rows
    traces = _by_build(new)
    # S2's first pass counts from the digits the ordered count wrote beside its keys
    for name in ("r101", "min_weight"):
        by_key = [src for _, src, _ in _BY_KEY.findall(traces[name])]
        assert "its writer's digits" in by_key, (name, traces[name][-1500:])
    # 101 bp: the left-over windows are appended to the k-mer records, so their writer hands over no counts
    assert [src for _, src, _ in _BY_KEY.findall(traces["r101"])][0] == "the keys", traces["r101"][-1500:]
    # three-word tiles over two-word mid tiles and k-mers
    assert sorted(int(nw) for _, nw, _, _ in _BY_HASH.findall(traces["k40"])) == [2, 2, 3], traces["k40"][-1500:]
    assert 3 in [int(nw) for _, nw, _, _ in _BY_HASH.findall(traces["k63"])], traces["k63"][-1500:]
    # the ordered count gave up on the crowded key prefixes and the records went on to the hash groups
    low = traces["low_complexity"]
    assert "counting by hash groups" in low and _BY_KEY.search(low) and [nw for _, nw, _, _ in _BY_HASH.findall(low)].count("1") == 1, low[-1500:]
