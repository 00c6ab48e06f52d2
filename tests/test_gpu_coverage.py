"""Unitig coverage on one GPU (katome_dev_shrink_coverage, katome_dev_contigs_gfa_coverage, katome_dev_gfa_coverage_arrays): per merged
edge the sum, smallest and largest k-mer count of the input edges on its path, against a model that looks every k-mer of every merged
edge up by its bases (tests/coverage_model.py), with the shrink result itself equal, array for array, to a twin builder's plain shrink;
and the GFA text whose KC is that sum, byte for byte against the model's restatement."""
import json
import os
import re

import numpy as np
import pytest

import coverage_model
import gfa_model
from helpers import ROOT, kmer_to_int, pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U32 = 2 ** 32 - 1
ARRAYS = ("edge_src", "edge_dst", "edge_weight", "edge_kmers", "edge_label_off", "edge_label", "node_key")


def _build(kd, packed, n, L, k, rc, first_seen=False):
    b = kd.Builder(k, rc, first_seen_order=first_seen)
    span = b.tile_span(L)
    if span > 1:
        b.insert_tiles(b.extract_tiles(packed, n, L, span), span)
    else:
        b.insert(b.extract_fixed(packed, n, L))
    b.finalize()
    return b


def _graph_host(b):
    """the graph as it stands -> (n_edges, edge_key rows of unsigned words, key_words, edge_weight)"""
    dg = b.graph()
    keys = dg.edge_key.cpu().numpy().view(np.uint64).reshape(dg.n_edges, dg.key_words).tolist()
    return dg.n_edges, keys, dg.key_words, dg.edge_weight.cpu().numpy().view(np.uint32).tolist()


def _coverage_host(dc):
    u = lambda t, dt: t.cpu().numpy().view(dt).tolist()
    return list(zip(u(dc.kmer_sum, np.uint64), u(dc.kmer_min, np.uint32), u(dc.kmer_max, np.uint32)))


def check_coverage(make, mode, k):
    """make() -> a finalized Builder, its stages run.  Everything every case asserts -> (builder, its coverage contigs, the coverage);
    the caller closes the builder"""
    b, twin = make(), make()
    n_edges, keys, nw, weights = _graph_host(b)
    dc, plain = b.shrink(mode, coverage=True), twin.shrink(mode)
    assert (dc.n_nodes, dc.n_edges, dc.label_bytes, dc.key_words) == (plain.n_nodes, plain.n_edges, plain.label_bytes, plain.key_words)
    for a in ARRAYS:
        if a == "edge_label_off" and dc.n_edges == 0:
            continue                               # (a shrink of no edges writes none: its one entry is not defined)
        assert torch.equal(getattr(dc, a).cpu(), getattr(plain, a).cpu()), a
    del plain
    twin.close()
    got = _coverage_host(dc)
    assert len(got) == dc.n_edges
    assert got == coverage_model.coverage(coverage_model.kmer_weights(keys, nw, weights), k, dc.sequences())
    assert sum(s for s, _, _ in got) == sum(weights)
    assert sum(dc.edge_kmers.cpu().tolist()) == n_edges
    return b, dc, got


# ---- the five synthetic read sets of the shrink tests -----------------------------------------------------------------------------
SETS = [(31, True, 4000, 100, 30000, 5e-3), (21, False, 3000, 80, 20000, 1e-2), (40, True, 2500, 103, 20000, 5e-3), (15, True, 3000, 60, 8000, 1e-2),
        (33, False, 2000, 150, 25000, 0.0)]
_packed = {}


def _synth(oracle, i):
    if i not in _packed:
        k, rc, n, L, glen, err = SETS[i]
        _packed[i] = pack_reads_ascii(oracle.synth_reads(0, n, L, glen, err, 0)).reshape(-1).copy()
    return torch.from_numpy(_packed[i]).cuda()


@pytest.mark.parametrize("variant", ["key_fast", "seen_exact", "seen_pruned_exact", "seen_fast"])
@pytest.mark.parametrize("i", range(len(SETS)))
def test_synthetic_reads(oracle, i, variant):
    from katome_amd import device as kd
    k, rc, n, L, glen, err = SETS[i]
    packed = _synth(oracle, i)

    def make():
        b = _build(kd, packed, n, L, k, rc, first_seen=variant != "key_fast")
        if variant == "seen_pruned_exact":
            b.remove_dead_paths()                # (indices out of age order from here on)
        return b
    b, dc, got = check_coverage(make, "exact" if variant.endswith("exact") else "fast", k)
    if variant == "seen_pruned_exact" and dc.n_edges == 0:
        assert SETS[i][0] == 40                    # (the first pruning leaves nothing of this set, as in the shrink tests: no edges, no coverage)
    else:
        assert dc.n_edges > 10 and any(mn < mx for _, mn, mx in got)
    del dc
    b.close()


@pytest.mark.parametrize("first_seen", [False, True])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures(golden_dir, i, first_seen):
    from katome_amd import device as kd
    from katome_amd.build import ingest_files, InputFileType
    pinned = json.load(open(os.path.join(golden_dir, "pinned.json")))
    path, k = os.path.join(golden_dir, pinned["fixtures"][i]), pinned["k"]
    r = ingest_files([path], InputFileType.Fastq, k)
    packed = torch.from_numpy(r["packed"].copy()).cuda()
    b, dc, got = check_coverage(lambda: _build(kd, packed, r["n_reads"], r["fixed_len"], k, False, first_seen), None, k)
    assert [dc.n_nodes, dc.n_edges] == pinned["shrink"]["counts"][i]
    del dc
    b.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("k,rc", [(11, False), (16, True), (31, True)])
def test_cycle_of_inner_vertices(k, rc, mode):
    """reads off one circle only, some of them twice: no vertex to start from; every edge of the cycle counts once"""
    from katome_amd import device as kd
    rng = np.random.default_rng(k)
    circle = "".join("ACGT"[c] for c in rng.integers(0, 4, 300))
    L = 60
    starts = list(range(0, 300, 7)) + [0, 7, 140, 140, 210]
    reads = np.array([[ord(c) for c in (circle + circle)[s:s + L]] for s in starts], dtype=np.uint8)
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b, dc, got = check_coverage(lambda: _build(kd, packed, len(reads), L, k, rc, first_seen=mode == "exact"), mode, k)
    assert dc.n_edges == (2 if rc else 1) and dc.edge_kmers.cpu().tolist() == [300] * dc.n_edges
    assert dc.edge_src.cpu().tolist() == dc.edge_dst.cpu().tolist()
    assert all(mn < mx and mn * 300 < s < mx * 300 for s, mn, mx in got)
    del dc
    b.close()


def test_single_self_loop():
    """one read of 40 x A at k = 11: one edge from AAAAAAAAAA to itself, seen 30 times"""
    from katome_amd import device as kd
    packed = torch.from_numpy(pack_reads_ascii(np.full((1, 40), ord("A"), np.uint8)).reshape(-1).copy()).cuda()
    for mode, first_seen in (("fast", False), ("exact", True)):
        b, dc, got = check_coverage(lambda: _build(kd, packed, 1, 40, 11, False, first_seen), mode, 11)
        assert dc.n_edges == 1 and got == [(30, 30, 30)] and dc.edge_kmers.cpu().tolist() == [1]
        del dc
        b.close()


def test_no_edges():
    """nothing long enough to give an edge went in: empty arrays, KATOME_OK, and a GFA of the header line alone"""
    from katome_amd import device as kd
    for mode, first_seen in (("fast", False), ("exact", True)):
        def make():
            b = kd.Builder(11, False, first_seen_order=first_seen)
            b.finalize()
            return b
        b, dc, got = check_coverage(make, mode, 11)
        assert dc.n_edges == 0 and got == [] and dc.kmer_sum.numel() == dc.kmer_min.numel() == dc.kmer_max.numel() == 0
        assert dc.gfa(coverage=True).bytes() == b"H\tVN:Z:1.0\n"
        del dc
        b.close()


def _s_fields(text):
    return [(name, seq, tags) for name, seq, tags in gfa_model.parse(text)[0]]


def test_weights_that_wrap_32_bits():
    """a line of 6 k-mers inserted with weights: the sum passes 32 bits, and the old KC (first weight x k-mers) is another number"""
    from katome_amd import device as kd
    k, rng = 11, np.random.default_rng(7)
    seq = "".join("ACGT"[c] for c in rng.integers(0, 4, k + 5))
    weights = [U32, 1, U32, 7, U32, U32]

    def make():
        b = kd.Builder(k, False)
        records = torch.from_numpy(np.array([kmer_to_int(seq[i:i + k]) for i in range(6)], np.uint64).view(np.int64).copy()).cuda()
        b.insert(records, torch.from_numpy(np.array(weights, np.uint32).view(np.int32).copy()).cuda())
        b.finalize()
        return b
    b, dc, got = check_coverage(make, "fast", k)
    assert dc.sequences() == [seq] and got == [(4 * U32 + 8, 1, U32)] and got[0][0] > U32
    assert dc.edge_weight.cpu().numpy().view(np.uint32).tolist() == [U32]
    with_cov, old = dc.gfa(coverage=True).bytes(), dc.gfa().bytes()
    (n1, s1, t1), (n0, s0, t0) = _s_fields(with_cov)[0], _s_fields(old)[0]
    assert (n1, s1) == (n0, s0) == (0, seq)
    assert t0 == {"LN": 16, "KC": 6 * U32, "ew": U32} and t1 == {"LN": 16, "KC": 4 * U32 + 8, "ew": U32, "mn": 1, "mx": U32}
    assert with_cov == old.replace(b"KC:i:%d\tew:i:%d\n" % (6 * U32, U32), b"KC:i:%d\tew:i:%d\tmn:i:1\tmx:i:%d\n" % (4 * U32 + 8, U32, U32))
    del dc
    b.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_one_long_unitig(mode):
    """a 3030-base random sequence at k = 31 read once, plus 200 reads of 100 bases over random parts of it: one walk of 3000 steps with
    the weights varying along it"""
    from katome_amd import device as kd
    k, rng = 31, np.random.default_rng(31)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 3030)]
    short = np.stack([seq[s:s + 100] for s in rng.integers(0, 3030 - 100 + 1, 200)])

    def make():
        b = kd.Builder(k, False)
        b.insert(b.extract_fixed(torch.from_numpy(pack_reads_ascii(seq[None, :]).reshape(-1).copy()).cuda(), 1, 3030))
        b.insert(b.extract_fixed(torch.from_numpy(pack_reads_ascii(short).reshape(-1).copy()).cuda(), 200, 100))
        b.finalize()
        return b
    b, dc, got = check_coverage(make, mode, k)
    assert dc.edge_kmers.cpu().tolist() == [3000] and got[0][1] == 1 and got[0][2] > 3 and got[0][0] == 3000 + 200 * 70
    del dc
    b.close()


def test_a_later_plain_shrink_drops_the_coverage(oracle):
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    k, rc, n, L, glen, err = SETS[1]
    b = _build(kd, _synth(oracle, 1), n, L, k, rc)
    dc = b.shrink("fast", coverage=True)
    assert dc.kmer_sum.numel() == dc.n_edges and dc.gfa(coverage=True).n_segments == dc.n_edges
    plain = b.shrink("fast")
    with pytest.raises(KatomePanic) as e:
        dc.gfa(coverage=True)
    assert e.value.name == "E_ARG"
    assert "last shrink was not a katome_dev_shrink_coverage" in e.value.message or "last katome_dev_shrink" in e.value.message
    for name in ("kmer_sum", "kmer_min", "kmer_max"):          # the earlier views are no longer handed out
        with pytest.raises(ValueError):
            getattr(dc, name)
    with pytest.raises(ValueError):                            # before the library is called
        plain.gfa(coverage=True)
    again = b.shrink("fast", coverage=True)
    with pytest.raises(ValueError):
        again.gfa(coverage=True, merge_strands=True)
    assert again.gfa(coverage=True).n_segments == again.n_edges
    del dc, plain, again
    b.close()


# ---- the GFA writer on hand-made arrays ---------------------------------------------------------------------------------------------
def _seqs(rng, lengths):
    return ["".join(rng.choice(list("ACGT"), n)) for n in lengths]


def _random_coverage(rng, k, weight, seqs):
    """consistent with the weights: min <= w <= max, min * kmers <= sum <= max * kmers"""
    mn = [int(rng.integers(0, w + 1)) for w in weight]
    mx = [int(rng.integers(w, 2 ** 32)) for w in weight]
    sm = [int(rng.integers(a * (len(s) - k + 1), b * (len(s) - k + 1) + 1, dtype=np.uint64)) for a, b, s in zip(mn, mx, seqs)]
    return sm, mn, mx


def _device_arrays(k, src, dst, weight, seqs, sm, mn, mx):
    """-> the arguments of kd.gfa_coverage_arrays after k and n_nodes, and label_bytes"""
    parts = [gfa_model.compress_edge(s) for s in seqs]
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    raw = b"".join(parts)
    lab = torch.from_numpy(np.frombuffer(raw + b"\0" * (16 + (-len(raw)) % 4), np.uint8).copy()).cuda()
    u32 = lambda a: torch.from_numpy(np.array(a, np.uint32).view(np.int32).copy()).cuda()
    u64 = lambda a: torch.from_numpy(np.array(a, np.uint64).view(np.int64).copy()).cuda()
    return (u64(src), u64(dst), u32(weight), u32([len(s) - k + 1 for s in seqs]), u64(sm), u32(mn), u32(mx), torch.from_numpy(off).cuda(), lab), len(raw)


def check_arrays(k, n_nodes, src, dst, weight, seqs, sm, mn, mx):
    from katome_amd import device as kd
    args, label_bytes = _device_arrays(k, src, dst, weight, seqs, sm, mn, mx)
    g = kd.gfa_coverage_arrays(k, n_nodes, *args, label_bytes=label_bytes)
    want, seg, first = coverage_model.gfa_coverage_text(k, src, dst, weight, [len(s) - k + 1 for s in seqs], seqs, sm, mn, mx)
    got = g.bytes()
    assert len(got) == g.text_bytes == len(want)
    assert got == want
    assert g.n_segments == len(seqs) and g.n_links == first[-1]
    assert g.segment_off.cpu().tolist() == seg and g.link_first.cpu().tolist() == first
    return got


def _case(name, k, rng):
    """-> (n_nodes, src, dst, weight, seqs): the cases of the plain writer's test, rebuilt here"""
    if name == "no_edges":
        return 3, [], [], [], []
    if name == "self_loop":
        return 1, [0], [0], [9], _seqs(rng, [k])
    if name == "every_pad":                        # a chain whose labels are k .. k + 9 bases long
        return 11, list(range(10)), list(range(1, 11)), [int(x) for x in rng.integers(1, 50, 10)], _seqs(rng, range(k, k + 10))
    if name == "hub":                              # 4 edges into vertex 4 and 4 out of it, in shuffled source order: 16 links
        src, dst = [0, 1, 2, 3, 4, 4, 4, 4], [4, 4, 4, 4, 5, 6, 7, 8]
        p = rng.permutation(8)
        return 9, [src[i] for i in p], [dst[i] for i in p], list(range(1, 9)), _seqs(rng, [int(x) for x in rng.integers(k, k + 30, 8)])
    if name == "many_segments":                    # names cross 10 / 100 / 1000; weights up to 2^32 - 1
        n = 1200
        lengths = [int(x) for x in rng.integers(k, k + 40, n)]
        lengths[1100] = 30000 + k - 1
        weight = [int(x) for x in rng.integers(1, 2 ** 32, n)]
        weight[0], weight[1100], weight[7] = U32, U32, 1
        return 600, [int(x) for x in rng.integers(0, 600, n)], [int(x) for x in rng.integers(0, 600, n)], weight, _seqs(rng, lengths)
    raise KeyError(name)


@pytest.mark.parametrize("k", [3, 11])
@pytest.mark.parametrize("name", ["no_edges", "self_loop", "every_pad", "hub", "many_segments"])
def test_writer_on_hand_made_arrays(name, k):
    rng = np.random.default_rng(len(name) * 131 + k)
    n_nodes, src, dst, weight, seqs = _case(name, k, rng)
    text = check_arrays(k, n_nodes, src, dst, weight, seqs, *_random_coverage(rng, k, weight, seqs))
    assert text.count(b"\tmx:i:") == len(seqs)


def _tile_bytes():
    """TILE of gfa_image.h: BLOCK * 16 * STORES output bytes per workgroup"""
    csrc = os.path.join(ROOT, "katome_amd", "csrc")
    image, common = open(os.path.join(csrc, "gfa_image.h")).read(), open(os.path.join(csrc, "common.h")).read()
    assert re.search(r"constexpr u32 TILE = BLOCK \* 16 \* STORES;", image)
    return int(re.search(r"constexpr int BLOCK = (\d+);", common).group(1)) * 16 * int(re.search(r"constexpr int STORES = (\d+);", image).group(1))


def test_tag_sweep():
    """500 segments of k + j bases, j = 0 .. 499: the tag block falls at every offset relative to the writer's tile edges; weights and
    maxima near 2^32, minima of 1 to 10 digits"""
    k, rng = 11, np.random.default_rng(24)         # (some 21 tile edges fall into these 177 kB: a seed with which they meet all four fields)
    n = 500
    seqs = _seqs(rng, [k + j for j in range(n)])
    weight = [U32 - int(x) for x in rng.integers(0, 1000, n)]
    mx = [min(U32, w + int(x)) for w, x in zip(weight, rng.integers(0, 1000, n))]
    mn = [int(rng.integers(10 ** (j % 10) if j % 10 else 0, min(10 ** (j % 10 + 1), w + 1))) for j, w in enumerate(weight)]      # j % 10 + 1 digits
    sm = [int(rng.integers(a * (j + 1), b * (j + 1) + 1, dtype=np.uint64)) for j, (a, b) in enumerate(zip(mn, mx))]
    assert {len(str(x)) for x in mn} == set(range(1, 11))
    text = check_arrays(k, n + 1, list(range(n)), list(range(1, n + 1)), weight, seqs, sm, mn, mx)
    tile = _tile_bytes()
    assert tile == 8192
    hit = set()
    for m in re.finditer(rb"\t(KC|ew|mn|mx):i:\d+", text):
        if (m.start() + 1) // tile != (m.end() - 1) // tile:      # a tile edge between two bytes of the field
            hit.add(m.group(1))
    assert hit == {b"KC", b"ew", b"mn", b"mx"}, hit


def test_fourteen_digit_kc():
    k, rng = 11, np.random.default_rng(14)
    seqs = _seqs(rng, [3000 + k - 1, k + 2])
    weight, mn, mx = [U32 - 5, 3], [U32 - 900, 1], [U32, 8]
    sm = [sum(int(x) for x in rng.integers(mn[0], mx[0] + 1, 3000)), 12]
    assert len(str(sm[0])) == 14
    check_arrays(k, 3, [0, 1], [1, 2], weight, seqs, sm, mn, mx)


def _raw_call(k, n_nodes, args, label_bytes, with_text):
    """katome_dev_gfa_coverage_arrays itself -> (status, message, n_links, text_bytes); with_text: not a size query"""
    import ctypes as C
    from katome_amd import _lib
    n_edges = args[7].numel() - 1
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    nl, nb = C.c_uint64(77), C.c_uint64(77)
    cap = 1 << 16
    seg, first, text = (torch.zeros(n_edges + 1, dtype=torch.int64).cuda(), torch.zeros(n_edges + 1, dtype=torch.int64).cuda(),
                        torch.zeros(cap, dtype=torch.uint8).cuda()) if with_text else (None, None, None)
    rc = _lib.lib().katome_dev_gfa_coverage_arrays(0, k, n_nodes, n_edges, *[p(t) for t in args], label_bytes, p(seg), p(first), p(text), cap if with_text else 0,
                                                   C.byref(nl), C.byref(nb), None)
    torch.cuda.synchronize()
    return _lib.STATUS[rc], _lib.last_error() if rc else "", nl.value, nb.value


def test_coverage_that_does_not_fit_is_refused():
    """each of them KATOME_E_ARG with its message, as a size query and with a text buffer alike; no size comes back"""
    k, rng = 5, np.random.default_rng(5)
    seqs = _seqs(rng, [7, 9, 12])                  # 3, 5 and 8 k-mers
    src, dst, weight = [0, 1, 2], [1, 2, 0], [10, 20, 30]
    good = dict(sm=[30, 100, 240], mn=[10, 20, 30], mx=[10, 20, 30])
    check_arrays(k, 3, src, dst, weight, seqs, **good)
    message = "gfa: a segment's coverage does not fit its weight and k-mer count"
    bad = {"min > weight": dict(mn=[10, 21, 30], sm=[30, 105, 240], mx=[10, 21, 30]), "max < weight": dict(mx=[10, 20, 29], mn=[10, 20, 29], sm=[30, 100, 232]),
           "sum < min * kmers": dict(sm=[30, 99, 240]), "sum > max * kmers": dict(sm=[30, 100, 241]),
           "sum > max * kmers, past 32 bits": dict(sm=[30, 100, 8 * U32 + 1], mx=[10, 20, U32])}
    for what, change in bad.items():
        a = dict(good)
        a.update(change)
        args, label_bytes = _device_arrays(k, src, dst, weight, seqs, a["sm"], a["mn"], a["mx"])
        for with_text in (False, True):
            assert _raw_call(k, 3, args, label_bytes, with_text) == ("E_ARG", message, 0, 0), (what, with_text)
    args, label_bytes = _device_arrays(k, src, dst, weight, seqs, **good)
    assert _raw_call(k, 3, args, label_bytes, True)[0] == "OK"
    for j in (4, 5, 6):                            # kmer_sum, kmer_min, kmer_max
        holed = list(args)
        holed[j] = None
        for with_text in (False, True):
            assert _raw_call(k, 3, holed, label_bytes, with_text) == ("E_ARG", "null argument", 0, 0), (j, with_text)


# ---- through the builder ---------------------------------------------------------------------------------------------------------------
def _host(dc):
    u = lambda t, dt: t.cpu().numpy().view(dt).tolist()
    return u(dc.edge_src, np.uint64), u(dc.edge_dst, np.uint64), u(dc.edge_weight, np.uint32), u(dc.edge_kmers, np.uint32), dc.sequences()


@pytest.mark.parametrize("first_seen", [False, True])
def test_contigs_gfa_coverage(oracle, first_seen):
    """DeviceContigs.gfa(coverage=True) against the model over the coverage arrays, and the plain gfa() right after it untouched"""
    from katome_amd import device as kd
    k, rc, n, L, glen, err = SETS[0]
    b = _build(kd, _synth(oracle, 0), n, L, k, rc, first_seen)
    dc = b.shrink(coverage=True)                   # (auto: fast by packed key, exact in first-seen order)
    src, dst, weight, kmers, seqs = _host(dc)
    sm, mn, mx = zip(*_coverage_host(dc))
    g = dc.gfa(coverage=True)
    want, seg, first = coverage_model.gfa_coverage_text(k, src, dst, weight, kmers, seqs, sm, mn, mx)
    assert g.bytes() == want and (g.n_segments, g.n_links, g.text_bytes) == (len(seqs), first[-1], len(want))
    assert g.segment_off.cpu().tolist() == seg and g.link_first.cpu().tolist() == first
    assert g.n_links > 10 and any(t["KC"] != t["ew"] * km for (_, _, t), km in zip(_s_fields(want), kmers))
    del g
    old = dc.gfa()
    want, seg, first = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)
    assert old.bytes() == want and old.segment_off.cpu().tolist() == seg and old.link_first.cpu().tolist() == first
    del old, dc
    b.close()
