"""Unitig coverage on the SHARDED graph, no gather (katome_dist_shrink_coverage, katome_dist_contigs_gfa_coverage, KATOME_FLAG_PATH_COVERAGE):
one process per rank sharing the card (thread ranks inside the host entries), against the one-GPU fast form's coverage of the same graph -- in first-seen order matched by
d_edge_head_id (the ranks' merged edges ordered by it ARE the one-GPU result), by packed key matched by sequence (the sharded head ids
count through the ranks' shares, not through the one-GPU key order) -- and the host entries on thread ranks."""
import os

import numpy as np
import pytest

import coverage_model
import gfa_model
from helpers import pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SETS = {"k31": (31, True, 4000, 100, 30000, 5e-3), "k40": (40, True, 2500, 103, 20000, 5e-3)}
THR = 2
# (read set, first-seen order, stage chain)
CASES = [(s, fs, chain) for s in SETS for fs, chain in ((False, ""), (True, ""), (True, "d"), (True, "dcwced"))]


def _case_name(s, fs, chain):
    return "%s_%s_%s" % (s, "seen" if fs else "key", chain or "plain")


def _reads(name):
    from oracle import oracle as o
    k, rc, n, L, glen, err = SETS[name]
    return o.synth_reads(0, n, L, glen, err, 0)


def _circle_reads():
    rng = np.random.default_rng(21)
    circle = "".join("ACGT"[c] for c in rng.integers(0, 4, 300))
    starts = list(range(0, 300, 7)) + [0, 7, 140, 140, 210]              # some reads twice: unequal weights along the circle
    return np.array([[ord(c) for c in (circle + circle)[s:s + 60]] for s in starts], dtype=np.uint8)


def _one_read():
    from oracle import oracle as o
    return o.synth_reads(3, 1, 34, 5000, 0.0, 0)


def _host(c):
    u = lambda t, dt: t.cpu().numpy().view(dt).copy()
    return dict(src=u(c.edge_src, np.uint64), dst=u(c.edge_dst, np.uint64), weight=u(c.edge_weight, np.uint32), kmers=u(c.edge_kmers, np.uint32),
                off=u(c.edge_label_off, np.int64), label=u(c.edge_label, np.uint8), node_key=u(c.node_key, np.uint64))


def _cov_host(c):
    u = lambda t, dt: t.cpu().numpy().view(dt).copy()
    return dict(kmer_sum=u(c.kmer_sum, np.uint64), kmer_min=u(c.kmer_min, np.uint32), kmer_max=u(c.kmer_max, np.uint32))


# ---- the one-GPU side ----------------------------------------------------------------------------------------------------------------
def _one_gpu(reads, k, rc, first_seen, chain, glen):
    """the one-GPU builder after the stage chain and its fast shrink with coverage -> (seqs, weight, kmers, coverage rows), in its order"""
    from katome_amd import device as kd
    n, L = reads.shape
    b = kd.Builder(k, rc, first_seen_order=first_seen)
    p = torch.from_numpy(np.concatenate([pack_reads_ascii(reads).reshape(-1), np.zeros(32, np.uint8)])).cuda()
    span = b.tile_span(L)
    if span > 1:
        b.insert_tiles(b.extract_tiles(p, n, L, span), span)
    else:
        b.insert(b.extract_fixed(p, n, L))
    b.finalize()
    for st in chain:
        {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.remove_weak_edges(THR), "e": lambda: b.standardize_edges(glen, THR)}[st]()
    dc = b.shrink("fast", coverage=True)
    h, cov = _host(dc), _cov_host(dc)
    out = (dc.sequences(), h["weight"].tolist(), h["kmers"].tolist(), list(zip(cov["kmer_sum"].tolist(), cov["kmer_min"].tolist(), cov["kmer_max"].tolist())))
    del dc
    b.close()
    return out


_ref = {}


def _reference(s, fs, chain):
    key = _case_name(s, fs, chain)
    if key not in _ref:
        k, rc, n, L, glen, err = SETS[s]
        _ref[key] = _one_gpu(_reads(s), k, rc, fs, chain, glen)
    return _ref[key]


# ---- one process per rank ----------------------------------------------------------------------------------------------------------------
def _sharded_builder(ks, comm, reads, k, rc, first_seen, chain, glen, rank, world):
    first, count = ks.shard_range(len(reads), world, rank)
    mine = pack_reads_ascii(reads[first:first + count]).reshape(-1) if count else np.zeros(0, np.uint8)      # (a rank may get no read)
    packed = torch.from_numpy(np.concatenate([mine, np.zeros(32, np.uint8)])).cuda()
    b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=first_seen)
    b.add_reads(packed, first, count, reads.shape[1], None, batch_reads=1024)
    b.finalize()
    for st in chain:
        {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.prune_weak_edges(THR), "e": lambda: b.standardize_edges(glen, THR)}[st]()
    return b


def _shrink_both_ways(b):
    """katome_dist_shrink, then katome_dist_shrink_coverage on the same builder: the same katome_dist_contigs, array for array -> what
    the parent compares"""
    del_first = b.shrink()                         # (the first shrink after a stage rebuilds the links: its bytes are not the shrink's alone)
    del del_first
    c = b.shrink()
    assert c.kmer_sum is None and c.kmer_min is None and c.kmer_max is None
    plain, plain_head = _host(c), c.edge_head_id.cpu().numpy().copy()
    counts = (c.n_edges, c.n_nodes, c.total_edges, c.total_nodes, c.label_bytes, c.key_words)
    sent = c.stats["bytes_sent"]
    del c
    c = b.shrink(coverage=True)
    assert (c.n_edges, c.n_nodes, c.total_edges, c.total_nodes, c.label_bytes, c.key_words) == counts
    got = _host(c)
    for name in plain:
        assert np.array_equal(plain[name], got[name]), name
    assert np.array_equal(plain_head, c.edge_head_id.cpu().numpy())
    assert c.kmer_sum.numel() == c.kmer_min.numel() == c.kmer_max.numel() == c.n_edges
    out = dict(got, head=plain_head, seqs=np.array(c.sequences(), dtype=object), sent=np.array([sent, c.stats["bytes_sent"]], np.uint64), **_cov_host(c))
    return c, out


def _rank_main(rank, world, what, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    # (the ranks meet through a file: a port picked in advance can be taken by another process before rank 0 listens on it)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = ks.Comm.over_torch(device=0)
        saved = {}

        def keep(prefix, out):
            for name, v in out.items():
                saved["%s.%s" % (prefix, name)] = v

        def refused(call, name, *words):
            try:
                call()
            except KatomePanic as e:
                assert e.name == name and all(w in str(e) for w in words), e
                return
            raise AssertionError("%s was not refused" % name)
        if what == "graphs":
            for s, fs, chain in CASES:
                k, rc, n, L, glen, err = SETS[s]
                b = _sharded_builder(ks, comm, _reads(s), k, rc, fs, chain, glen, rank, world)
                c, out = _shrink_both_ways(b)
                keep(_case_name(s, fs, chain), out)
                del c
                b.close()
        else:
            assert what == "extras"
            # the circle: the cycle of inner vertices crosses the ranks
            b = _sharded_builder(ks, comm, _circle_reads(), 21, True, True, "", 0, rank, world)
            c, out = _shrink_both_ways(b)
            keep("circle", out)
            del c
            b.close()
            # the failure knob: every rank gets the error and no coverage is left behind
            k, rc, n, L, glen, err = SETS["k31"]
            b = _sharded_builder(ks, comm, _reads("k31"), k, rc, True, "", glen, rank, world)
            c = b.shrink(coverage=True)
            del c
            os.environ["KATOME_DIST_SHRINK_FAIL"] = "1"
            refused(lambda: b.shrink(coverage=True), "E_UNSUPPORTED", "rank 1")
            del os.environ["KATOME_DIST_SHRINK_FAIL"]
            refused(lambda: b.contigs_gfa(coverage=True), "E_ARG")                       # (no shrink result at all after the failure)
            b.close()
            b = _sharded_builder(ks, comm, _reads("k31"), k, rc, True, "", glen, rank, world)
            c = b.shrink()
            refused(lambda: b.contigs_gfa(coverage=True), "E_ARG", "katome_dist_shrink_coverage")      # a coverage-less last shrink: on every rank
            plain = b.contigs_gfa()                                                      # ... while the plain text is there
            assert plain.total_segments == c.total_edges
            del plain, c
            # the GFA with coverage and its file
            c, out = _shrink_both_ways(b)
            g = b.contigs_gfa(coverage=True)
            u = lambda t, dt: t.cpu().numpy().view(dt).copy()
            out.update(s_text=u(g.s_text, np.uint8), l_text=u(g.l_text, np.uint8), total_text=np.array([g.total_text_bytes, g.total_links], np.uint64))
            b.save_gfa(g, os.path.join(out_dir, "coverage.gfa"))
            keep("gfa", out)
            c2 = b.shrink()                                                              # the later plain shrink drops the coverage and makes the text stale
            refused(lambda: b.save_gfa(g, os.path.join(out_dir, "stale.gfa")), "E_ARG")
            refused(lambda: b.contigs_gfa(coverage=True), "E_ARG", "katome_dist_shrink_coverage")
            del c, c2, g
            b.close()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **saved)
        comm.close()
    finally:
        dist.destroy_process_group()


def _spawn(world, what, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_rank_main, args=(world, what, str(tmp_path)), nprocs=world, join=True)
    return [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r), allow_pickle=True) for r in range(world)]


def _rows(parts, prefix):
    cat = lambda name: np.concatenate([p["%s.%s" % (prefix, name)] for p in parts])
    return cat("seqs").tolist(), cat("weight").tolist(), cat("kmers").tolist(), list(zip(cat("kmer_sum").tolist(), cat("kmer_min").tolist(), cat("kmer_max").tolist())), cat("head")


def _same_as_one_gpu(parts, prefix, ref, by_head, may_be_empty=False):
    seqs, weight, kmers, cov, head = _rows(parts, prefix)
    ref_seqs, ref_weight, ref_kmers, ref_cov = ref
    assert len(seqs) == len(ref_seqs) and (len(seqs) > 0 or may_be_empty)
    if by_head:                                    # first-seen order: ordered by head id the ranks' edges are the one-GPU result
        order = np.argsort(head, kind="stable").tolist()
        assert len(set(head.tolist())) == len(order)
        assert [seqs[i] for i in order] == ref_seqs and [weight[i] for i in order] == ref_weight and [kmers[i] for i in order] == ref_kmers
        assert [cov[i] for i in order] == ref_cov
    else:
        assert sorted(zip(seqs, weight, kmers, cov)) == sorted(zip(ref_seqs, ref_weight, ref_kmers, ref_cov))
    assert all(mn <= w <= mx and mn * km <= s <= mx * km for w, km, (s, mn, mx) in zip(weight, kmers, cov))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_process_ranks_equal_one_gpu(oracle, tmp_path, world):
    """both read sets, by packed key and in first-seen order straight after finalize, in first-seen order also after remove_dead_paths
    and after "dcwced": every rank's coverage is the one-GPU fast form's, and katome_dist_contigs is katome_dist_shrink's (asserted on
    the ranks)"""
    parts = _spawn(world, "graphs", tmp_path)
    for s, fs, chain in CASES:
        name = _case_name(s, fs, chain)
        # (the first pruning leaves nothing of the k = 40 set, as in the shrink tests: ranks without edges, empty coverage)
        _same_as_one_gpu(parts, name, _reference(s, fs, chain), by_head=fs, may_be_empty=s == "k40" and "d" in chain)
        seqs, weight, kmers, cov, _ = _rows(parts, name)
        if not seqs:
            continue
        if "c" in chain:                           # standardize_contigs gives every edge of a path one weight
            assert all(mn == mx == w and sm == w * km for w, km, (sm, mn, mx) in zip(weight, kmers, cov)), name
        else:
            assert any(mn < mx for _, mn, mx in cov), name
        if world > 1:                              # the extra exchange is counted: one more 16-byte record per non-head edge that travels
            for p in parts:
                plain_sent, cov_sent = (int(x) for x in p[name + ".sent"])
                assert cov_sent >= plain_sent, name
            assert sum(int(p[name + ".sent"][1]) for p in parts) > sum(int(p[name + ".sent"][0]) for p in parts), name


def test_one_read_on_eight_ranks(oracle, tmp_path):
    """four 31-mers on eight thread ranks (the host entry): most ranks hold nothing, and the one unitig's coverage comes out whole"""
    from katome_amd.build import GpuUnitigs
    reads = _one_read()
    out = str(tmp_path / "one.gfa")
    u, _ = GpuUnitigs.gfa_from_packed(pack_reads_ascii(reads).reshape(-1).copy(), 1, 34, reverse_complement=False, output_file=out, k=31, n_devices=8,
                                      ranks_share_device=True, coverage=True)
    assert open(out, "rb").read() == b"H\tVN:Z:1.0\nS\t0\t%s\tLN:i:34\tKC:i:4\tew:i:1\tmn:i:1\tmx:i:1\n" % reads[0].tobytes()
    assert (u.n_segments, u.n_links, u.n_devices, u.total_bases) == (1, 0, 8, 34)


@pytest.mark.timeout(600)
def test_circle_failure_and_gfa_on_three_ranks(oracle, tmp_path):
    parts = _spawn(3, "extras", tmp_path)
    # the circle, cut where the one-GPU fast form cuts it
    ref = _one_gpu(_circle_reads(), 21, True, True, "", 0)
    _same_as_one_gpu(parts, "circle", ref, by_head=True)
    seqs, weight, kmers, cov, _ = _rows(parts, "circle")
    assert kmers == [300, 300] and all(mn < mx for _, mn, mx in cov)
    # (the failure knob and the refusals are asserted on the ranks)
    assert not os.path.exists(os.path.join(str(tmp_path), "stale.gfa"))
    # the file: the model over the ranks' arrays put together in rank order
    k = SETS["k31"][0]
    cat = lambda name: np.concatenate([p["gfa." + name] for p in parts])
    seqs = cat("seqs").tolist()
    want, _, first = coverage_model.gfa_coverage_text(k, cat("src"), cat("dst"), cat("weight"), cat("kmers"), seqs, cat("kmer_sum"), cat("kmer_min"),
                                                      cat("kmer_max"))
    whole = b"".join(bytes(p["gfa.s_text"]) for p in parts) + b"".join(bytes(p["gfa.l_text"]) for p in parts)
    assert whole == want and len(seqs) > 10 and first[-1] > 10
    assert open(os.path.join(str(tmp_path), "coverage.gfa"), "rb").read() == want
    assert all(tuple(int(x) for x in p["gfa.total_text"]) == (len(want), first[-1]) for p in parts)
    _same_as_one_gpu(parts, "gfa", _reference("k31", True, ""), by_head=True)


# ---- the host entries: KATOME_FLAG_PATH_COVERAGE on thread ranks -----------------------------------------------------------------------
def _s_rows(data):
    segments, lks = gfa_model.parse(data)
    return sorted((seq, t["KC"], t["ew"], t["mn"], t["mx"]) for _, seq, t in segments), len(lks)


@pytest.mark.timeout(300)
def test_unitigs_gfa_with_the_flag(oracle, tmp_path):
    from katome_amd import device as kd
    from katome_amd.build import GpuUnitigs
    k, rc, n, L, glen, err = SETS["k31"]
    reads = _reads("k31")
    packed = pack_reads_ascii(reads).reshape(-1).copy()

    def run(n_devices, coverage):
        out = str(tmp_path / ("u%d_%d.gfa" % (n_devices, coverage)))
        u, _ = GpuUnitigs.gfa_from_packed(packed, n, L, reverse_complement=rc, output_file=out, k=k, first_seen_order=True, n_devices=n_devices,
                                          ranks_share_device=n_devices > 1, coverage=coverage)
        data = open(out, "rb").read()
        assert u.text_bytes == len(data) and u.n_devices == n_devices
        return u, data
    b = kd.Builder(k, rc, first_seen_order=True)
    p = torch.from_numpy(np.concatenate([packed, np.zeros(32, np.uint8)])).cuda()
    span = b.tile_span(L)
    if span > 1:
        b.insert_tiles(b.extract_tiles(p, n, L, span), span)
    else:
        b.insert(b.extract_fixed(p, n, L))
    b.finalize()
    dc = b.shrink("fast", coverage=True)
    with_cov = dc.gfa(coverage=True).bytes()
    plain = dc.gfa().bytes()
    del dc
    b.close()
    u1, one = run(1, True)
    assert one == with_cov                         # one device: the device text of katome_dev_contigs_gfa_coverage
    want_rows, want_links = _s_rows(one)
    assert len(want_rows) > 10 and want_links == u1.n_links > 10 and any(kc != ew * (len(seq) - k + 1) for seq, kc, ew, _, _ in want_rows)
    for n_devices in (2, 3):
        u, data = run(n_devices, True)
        assert _s_rows(data) == (want_rows, want_links) and u.n_links == want_links and u.n_segments == len(want_rows)
    assert run(1, False)[1] == plain               # without the flag: today's file, byte for byte
    assert b"mn:i:" not in plain and b"mn:i:" not in run(3, False)[1]
