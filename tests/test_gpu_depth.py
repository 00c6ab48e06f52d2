"""katome_dev_depth / katome_dev_depth_arrays on the GPU, every case element for element against tests/depth_model.py: hand-made key
sets through the arrays entry at the word boundaries of k, and builders in both numberings (the reads against their own graph, the
unitigs against shrink's coverage, the kept index across every stage that changes the edges)."""
import ctypes as C

import numpy as np
import pytest

import depth_model as dm
from helpers import int_to_kmer, int_to_words, pack_reads_ascii, revcomp_str
from test_gpu_coverage import SETS, _build, _graph_host

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE = 4096                    # windows a workgroup takes (depth.hip DEPTH_TILE)
KS = [3, 31, 32, 33, 63]
U32 = 2 ** 32 - 1


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def _rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _pack(queries):
    """strings of ACGT -> (uint8 tensor, byte_off, lens): 4 bases per byte, every sequence starting on a byte"""
    parts, off = [], [0]
    for q in queries:
        if q:
            parts.append(pack_reads_ascii(np.frombuffer(q.encode(), np.uint8).reshape(1, -1)).reshape(-1))
        off.append(off[-1] + (len(q) + 3) // 4)
    raw = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return raw, off[:-1], [len(q) for q in queries]


def _ascii(queries, gap=b"\n"):
    """any strings -> one text with `gap` between the sequences (and in front: offset 0 is not a sequence's)"""
    text, off = bytearray(gap), []
    for q in queries:
        off.append(len(text))
        text += q.encode() + gap
    return np.frombuffer(bytes(text), np.uint8), off, [len(q) for q in queries]


def _dev(raw, off, lens):
    return (torch.from_numpy(np.ascontiguousarray(raw).copy()).cuda() if len(raw) else torch.empty(0, dtype=torch.uint8, device="cuda"),
            torch.tensor(off, dtype=torch.int64, device="cuda"), torch.tensor(lens, dtype=torch.int32, device="cuda"))


def _keys_dev(key_ints, k):
    nw = 1 if k <= 31 else 2
    a = np.array([int_to_words(v, nw) for v in key_ints], dtype=np.uint64).reshape(-1)
    return torch.from_numpy(a.view(np.int64).copy()).cuda() if len(key_ints) else torch.empty(0, dtype=torch.int64, device="cuda")


def _weights_dev(weights):
    return torch.from_numpy(np.array(weights, dtype=np.uint32).view(np.int32).copy()).cuda() if len(weights) else torch.empty(0, dtype=torch.int32, device="cuda")


def _host(r):
    """a result (DeviceDepth or depth_arrays' dict) -> the model's dict of lists"""
    g = (lambda f: r[f]) if isinstance(r, dict) else (lambda f: getattr(r, f))
    u = lambda t, dt: t.cpu().numpy().view(dt).tolist()
    out = {f: int(g(f)) for f in ("n_seqs", "n_windows", "n_present", "n_invalid", "weight_sum", "n_edges", "n_edges_hit")}
    for f in ("seq_present", "seq_invalid", "seq_sum", "seq_window_off"):
        out[f] = u(g(f), np.uint64)
    for f in ("seq_min", "seq_max"):
        out[f] = u(g(f), np.uint32)
    out["window_edge"] = u(g("window_edge"), np.uint64) if g("window_edge") is not None else None
    out["edge_hits"] = u(g("edge_hits"), np.uint32) if g("edge_hits") is not None else None
    return out


def _assert_equal(got, want, windows=True, hits=True):
    for f in ("n_seqs", "n_windows", "n_present", "n_invalid", "weight_sum", "n_edges", "seq_window_off", "seq_present", "seq_invalid", "seq_sum",
              "seq_min", "seq_max"):
        assert got[f] == want[f], f
    if windows:
        assert got["window_edge"] == want["window_edge"]
    else:
        assert got["window_edge"] is None
    if hits:
        assert got["edge_hits"] == [want["edge_hits"].get(e, 0) for e in range(want["n_edges"])]
        assert got["n_edges_hit"] == want["n_edges_hit"] and sum(got["edge_hits"]) == got["n_present"]
    else:
        assert got["edge_hits"] is None and got["n_edges_hit"] == 0


def _arrays_case(k, key_ints, weights, queries, encoding="packed", either=False, windows=True, hits=True):
    from katome_amd import device as kd
    edges = {int_to_kmer(v, k): (e, w) for e, (v, w) in enumerate(zip(key_ints, weights))}
    want = dm.depth(edges, k, queries, either)
    seq, off, lens = _dev(*(_pack(queries) if encoding == "packed" else _ascii(queries)))
    got = _host(kd.depth_arrays(k, _keys_dev(key_ints, k), _weights_dev(weights), seq, off, lens, encoding, either, windows, hits))
    _assert_equal(got, want, windows, hits)
    return got


def _graph(rng, k, n):
    """n distinct random keys (fewer where 4^k is small), shuffled, with a weight of 0 and one of 2^32 - 1 among them"""
    n = min(n, 4 ** k * 5 // 8)
    keys = set()
    while len(keys) < n:
        keys.add(int.from_bytes(rng.bytes(16), "little") % 4 ** k)
    keys = list(keys)
    rng.shuffle(keys)
    weights = [int(w) for w in rng.integers(1, 1000, n)]
    if n >= 2:
        weights[0], weights[1] = 0, U32
    return keys, weights


def _seeded(rng, k, keys, n_bases):
    """n_bases bases: random, with key strings laid in (so that some windows are present)"""
    s = []
    while sum(map(len, s)) < n_bases:
        s.append(int_to_kmer(keys[int(rng.integers(0, len(keys)))], k) if keys and rng.random() < 0.5 else _rand_seq(rng, int(rng.integers(1, 2 * k))))
    return "".join(s)[:n_bases]


# ---- the arrays entry: hand-made key sets ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=KS)
def world(request):
    k = request.param
    rng = np.random.default_rng(1000 + k)
    keys, weights = _graph(rng, k, 5000)
    return k, rng, keys, weights


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("either", [False, True])
def test_mixed_queries(world, order, either):
    k, rng, keys, weights = world
    if order != "shuffled":
        pairs = sorted(zip(keys, weights), reverse=order == "descending")
        keys, weights = [p[0] for p in pairs], [p[1] for p in pairs]
    rng = np.random.default_rng(k)
    cut = [int_to_kmer(v, k) for v in keys[:60]]
    queries = [_rand_seq(rng, n) for n in (k - 1, k, k + 1, k + 2, k + 3, k + 4, 0, 1)]           # (k .. k + 3 bases: every filling of the last packed byte)
    queries += [_seeded(rng, k, keys, 3 * TILE + 100 + k)]                                         # one sequence over at least three tiles ...
    queries += [_seeded(rng, k, keys, k + 2) for _ in range(300)]                                  # ... many short ones inside a tile
    queries += [_seeded(rng, k, keys, TILE + 500), _seeded(rng, k, keys, k + 5), _seeded(rng, k, keys, TILE + 777)]    # long, short, long
    queries += cut + [revcomp_str(s) for s in cut]                                                 # present; absent or bit 63
    queries += ["", _rand_seq(rng, k - 1)]                                                         # (nothing behind the last window)
    got = _arrays_case(k, keys, weights, queries, "packed", either)
    assert got["n_present"] >= 60 and got["n_present"] < got["n_windows"]
    if either:
        assert sum(1 for v in got["window_edge"] if v >> 63 and v < dm.INVALID) >= (1 if k > 3 else 0)
    first_cut = len(queries) - 2 - 2 * len(cut)
    assert got["seq_present"][first_cut:first_cut + len(cut)] == [1] * len(cut)


@pytest.mark.parametrize("extra", [0, 1])
def test_last_sequence_ends_on_a_tile_boundary(world, extra):
    k, rng, keys, weights = world
    rng = np.random.default_rng(7 * k + extra)
    queries = [_seeded(rng, k, keys, k + 9) for _ in range(50)] + [_seeded(rng, k, keys, TILE + 3)]
    have = sum(len(q) - k + 1 for q in queries)
    queries.append(_seeded(rng, k, keys, 2 * TILE - have + k - 1 + extra))        # exactly two tiles of windows, or one window more
    got = _arrays_case(k, keys, weights, queries)
    assert got["n_windows"] == 2 * TILE + extra


def test_more_sequences_in_a_tile_than_lds_slots(world):
    """sequences of one window each (and empty ones between them): the ones past a tile's LDS slots go to the outputs' atomics"""
    k, rng, keys, weights = world
    rng = np.random.default_rng(11 * k)
    queries = []
    for i in range(TILE + 700):
        queries.append(int_to_kmer(keys[i % len(keys)], k) if i % 3 else _rand_seq(rng, k))
        if i % 5 == 0:
            queries.append(_rand_seq(rng, k - 1))
    _arrays_case(k, keys, weights, queries)
    _arrays_case(k, keys, weights, queries, "ascii", True)


@pytest.mark.parametrize("n_keys", [0, 1, 2])
def test_tiny_graphs(world, n_keys):
    k, rng, keys, weights = world
    keys, weights = keys[:n_keys], [0, U32][:n_keys]
    rng = np.random.default_rng(k + n_keys)
    queries = [int_to_kmer(v, k) for v in keys] + [revcomp_str(int_to_kmer(v, k)) for v in keys] + [_rand_seq(rng, 3 * k), _rand_seq(rng, k - 1)]
    for either in (False, True):
        got = _arrays_case(k, keys, weights, queries, "packed", either)
        assert got["n_present"] >= n_keys
    if n_keys == 2:
        assert got["seq_min"][:2] == [0, U32] and got["seq_max"][:2] == [0, U32] and got["seq_sum"][:2] == [0, U32]


def test_no_sequences_and_none_long_enough(world):
    k, rng, keys, weights = world
    got = _arrays_case(k, keys, weights, [])
    assert got["n_windows"] == 0 and got["seq_window_off"] == [0]
    got = _arrays_case(k, keys, weights, ["A" * (k - 1), "", "AC"])
    assert got["n_windows"] == 0 and got["seq_min"] == [U32] * 3 and got["seq_max"] == [0] * 3


def test_ascii_bytes_that_are_no_bases(world):
    k, rng, keys, weights = world
    rng = np.random.default_rng(13 * k)
    n = 3 * k + 7
    queries = []
    for places in ([0], [k - 1], [k], [n - 1], [k + 1, 2 * k - 1], [0, n - 1]):           # (the pair: fewer than k apart)
        s = list(_seeded(rng, k, keys, n))
        for p in places:
            s[p] = "N"
        queries.append("".join(s))
    lower = _seeded(rng, k, keys, n)
    queries += [lower[:k + 2] + lower[k + 2].lower() + lower[k + 3:], lower.lower(), int_to_kmer(keys[0], k) + "n" + int_to_kmer(keys[1], k)]
    queries += [_seeded(rng, k, keys, 2 * TILE + 50)[:TILE] + "N" + _seeded(rng, k, keys, TILE)]        # an N where a lane starts over
    for either in (False, True):
        got = _arrays_case(k, keys, weights, queries, "ascii", either)
        assert got["seq_invalid"][:6] == [1, k, k, 1, 2 * k - 2, 2]          # (the windows that cover one of the places)
        assert got["seq_present"][-2] == 2 and got["seq_invalid"][-2] == k
    # the same bases packed and as text: the same answer
    clean = [_seeded(rng, k, keys, n) for _ in range(20)]
    a, p = _arrays_case(k, keys, weights, clean, "ascii"), _arrays_case(k, keys, weights, clean, "packed")
    assert a == p


def test_flag_combinations(world):
    k, rng, keys, weights = world
    rng = np.random.default_rng(17 * k)
    queries = [_seeded(rng, k, keys, TILE + 50)] + [_seeded(rng, k, keys, k + 3) for _ in range(40)]
    full = _arrays_case(k, keys, weights, queries, windows=True, hits=True)
    for windows, hits in ((False, False), (True, False), (False, True)):
        got = _arrays_case(k, keys, weights, queries, windows=windows, hits=hits)
        for f in ("seq_present", "seq_invalid", "seq_sum", "seq_min", "seq_max", "seq_window_off", "n_present", "weight_sum"):
            assert got[f] == full[f]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(fn, name, *words):
    from katome_amd.build import KatomePanic
    with pytest.raises(KatomePanic) as e:
        fn()
    assert e.value.name == name, e.value.message
    for w in words:
        assert w in e.value.message, e.value.message


def test_refusals():
    from katome_amd import _lib, device as kd
    k = 5
    keys, weights = [1, 2, 3], [1, 1, 1]
    dk, dw = _keys_dev(keys, k), _weights_dev(weights)
    seq, off, lens = _dev(*_pack(["ACGTACGT", "ACGTACG", "ACGTAC"]))
    assert off.tolist() == [0, 2, 4]
    call = lambda **kw: kd.depth_arrays(k, kw.get("dk", dk), kw.get("dw", dw), seq, kw.get("off", off), lens, kw.get("encoding", "packed"),
                                         flags=kw.get("flags"))
    _refused(lambda: call(off=torch.tensor([0, 4, 2], dtype=torch.int64, device="cuda")), "E_ARG", "does not ascend", "sequence 2")
    _refused(lambda: call(off=torch.tensor([0, 2, 5], dtype=torch.int64, device="cuda")), "E_ARG", "runs past seq_bytes", "sequence 2")
    _refused(lambda: call(off=torch.tensor([0, 2, 1 << 62], dtype=torch.int64, device="cuda")), "E_ARG", "runs past seq_bytes")
    _refused(lambda: call(encoding="ascii"), "E_ARG", "runs past seq_bytes", "sequence 0")           # 8 bases in 6 bytes
    _refused(lambda: call(dk=_keys_dev([7, 3, 9, 3], k), dw=_weights_dev([1, 1, 1, 1])), "E_ARG", "keys 1 and 3 are equal")
    _refused(lambda: call(flags=8), "E_ARG", "unknown flag bits")
    _refused(lambda: call(encoding=2), "E_ARG", "unknown encoding")
    b = kd.Builder(k, False)
    _refused(lambda: b.depth(seq, off, lens), "E_ARG", "katome_dev_finalize first")
    b.finalize()
    assert _lib.lib().katome_dev_depth(b._h, 0, 0, kd._ptr(seq), seq.numel(), kd._ptr(off), kd._ptr(lens), 3, None, None) == -7      # NULL out
    assert "null argument" in _lib.last_error()
    r = b.depth(seq, off, lens, windows=True, edge_hits=True)                                       # a graph without edges: zero results
    assert (r.n_edges, r.n_windows, r.n_present, r.n_edges_hit) == (0, 4 + 3 + 2, 0, 0) and r.seq_min.tolist() == [-1] * 3
    assert r.window_edge.tolist() == [-1] * 9
    del r
    b.close()


# ---- builders ----------------------------------------------------------------------------------------------------------------------
_reads = {}


def _set(oracle, i):
    """synthetic read set i of the coverage tests -> (its strings, the packed reads on the device, byte_off, lens)"""
    if i not in _reads:
        k, rc, n, L, glen, err = SETS[i]
        rows = oracle.synth_reads(0, n, L, glen, err, 0)
        _reads[i] = ([bytes(r).decode() for r in rows], pack_reads_ascii(rows).reshape(-1).copy())
    k, rc, n, L, glen, err = SETS[i]
    strings, packed = _reads[i]
    stride = (L + 3) // 4
    return (strings, torch.from_numpy(packed).cuda(), torch.arange(n, dtype=torch.int64, device="cuda") * stride,
            torch.full((n,), L, dtype=torch.int32, device="cuda"))


def _model(b, k, queries, either=False):
    n_edges, key_rows, nw, weights = _graph_host(b)
    return dm.depth(dm.edge_dict(key_rows, k, weights), k, queries, either), weights


@pytest.mark.parametrize("first_seen", [False, True])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_reads_against_their_own_graph(oracle, i, first_seen):
    from katome_amd import device as kd
    k, rc, n, L, glen, err = SETS[i]
    strings, packed, off, lens = _set(oracle, i)
    b = _build(kd, packed, n, L, k, rc, first_seen)
    want, weights = _model(b, k, strings)
    assert b.depth_index_bytes() == 0
    got = _host(b.depth(packed, off, lens, windows=True, edge_hits=True))
    _assert_equal(got, want)
    assert got["n_present"] == got["n_windows"] == n * (L - k + 1)
    if not rc:
        assert got["edge_hits"] == weights              # (an edge's weight is how often its k-mer occurs in the reads)
    held = b.depth_index_bytes()
    n_edges = got["n_edges"]
    assert 0 < held and (held > n_edges * 12 if first_seen else held < n_edges * 4)      # a sorted copy only where the keys do not ascend
    again = _host(b.depth(packed, off, lens, windows=True, edge_hits=True))              # from the kept index; hits start at zero again
    assert again == got and b.depth_index_bytes() == held
    if rc:      # both strands are edges: the forward lookup already finds everything
        assert _host(b.depth(packed, off, lens, either_strand=True, windows=True, edge_hits=True)) == got
    summary = _host(b.depth(packed, off, lens))
    _assert_equal(summary, want, windows=False, hits=False)
    b.close()


@pytest.mark.parametrize("first_seen", [False, True])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_unitigs_against_shrink_coverage(oracle, i, first_seen):
    """every k-mer of every unitig is an edge of the graph it was shrunk from, once; sums, minima and maxima are shrink's own"""
    from katome_amd import device as kd
    k, rc, n, L, glen, err = SETS[i]
    strings, packed, off, lens = _set(oracle, i)
    b = _build(kd, packed, n, L, k, rc, first_seen)
    dc = b.shrink("fast", coverage=True)
    r = kd.DeviceDepth.of_text(b, dc.text("plain"), edge_hits=True)
    n_edges = b.graph().n_edges
    assert r.n_present == r.n_windows == n_edges and r.n_invalid == 0
    assert torch.equal(r.seq_present.cpu(), dc.edge_kmers.cpu().to(torch.int64))
    assert torch.equal(r.seq_sum.cpu(), dc.kmer_sum.cpu()) and torch.equal(r.seq_min.cpu(), dc.kmer_min.cpu()) and torch.equal(r.seq_max.cpu(), dc.kmer_max.cpu())
    assert r.n_edges_hit == r.n_edges == n_edges and r.edge_hits.cpu().tolist() == [1] * n_edges
    del r, dc
    b.close()


def test_kept_index_does_not_go_stale(oracle):
    from katome_amd import device as kd
    k, rc, n, L, glen, err = SETS[0]
    strings, packed, off, lens = _set(oracle, 0)
    b = _build(kd, packed, n, L, k, rc, first_seen=True)
    query = lambda: _host(b.depth(packed, off, lens, windows=True, edge_hits=True))
    before = query()
    _assert_equal(before, _model(b, k, strings)[0])
    b.remove_dead_paths()
    pruned = query()
    _assert_equal(pruned, _model(b, k, strings)[0])
    assert pruned["n_edges"] < before["n_edges"] and pruned["n_present"] < before["n_present"]
    b.remove_weak_edges(2)
    weak = query()
    _assert_equal(weak, _model(b, k, strings)[0])
    assert weak["n_edges"] < pruned["n_edges"]
    held = b.depth_index_bytes()
    b.standardize_contigs()                      # weights only: the index stays, the weights follow
    assert b.depth_index_bytes() == held
    std = query()
    _assert_equal(std, _model(b, k, strings)[0])
    assert std["window_edge"] == weak["window_edge"] and std["seq_sum"] != weak["seq_sum"]
    b.standardize_edges(glen, 0)
    _assert_equal(query(), _model(b, k, strings)[0])
    b.close()


def test_weak_edges_before_finalize_on_a_by_key_builder(oracle):
    from katome_amd import device as kd
    k, rc, n, L, glen, err = SETS[1]
    strings, packed, off, lens = _set(oracle, 1)
    b = kd.Builder(k, rc)
    b.insert(b.extract_fixed(packed, n, L))
    b.remove_weak_edges(2)
    b.finalize()
    got = _host(b.depth(packed, off, lens, windows=True, edge_hits=True))
    _assert_equal(got, _model(b, k, strings)[0])
    assert 0 < got["n_present"] < got["n_windows"]
    # a builder is finalized once: more reads after it are refused, so there is no second finalize whose index could go stale
    _refused(lambda: b.insert(b.extract_fixed(packed, n, L)), "E_ARG", "already finalized")
    assert _host(b.depth(packed, off, lens, windows=True, edge_hits=True)) == got
    b.close()


def test_assembly_against_the_unpruned_graph(oracle):
    """collapse()'s contigs spell paths of the graph: every window of the assembly is an edge of a twin's unpruned graph (error rate 0)"""
    from katome_amd import device as kd
    k, rc, n, L, glen, err = SETS[4]
    assert err == 0.0
    strings, packed, off, lens = _set(oracle, 4)
    b, twin = _build(kd, packed, n, L, k, rc, first_seen=True), _build(kd, packed, n, L, k, rc, first_seen=False)
    a = b.collapse("fasta")
    r = kd.DeviceDepth.of_text(twin, a, windows=True)
    assert r.n_seqs == a.n_contigs > 0 and r.n_windows == sum(max(0, l - k + 1) for l in a.lengths()) > 0
    assert r.n_present == r.n_windows and r.n_invalid == 0
    want, _ = _model(twin, k, a.contigs())
    _assert_equal(_host(r), want, hits=False)
    del r, a
    b.close()
    twin.close()
