"""The unitig graph of the sharded shrink as GFA 1, no gather (katome_amd/csrc/dist_gfa.hip; gfa.hip's writer in its numbered form):
the numbered writer on hand-made arrays, the join and the file on process ranks, the host entry katome_unitigs_gfa_* on thread
ranks, the edge cases of the join and the failures.  The oracle throughout: the file is, byte for byte, what gfa_model.gfa_text
gives for the ranks' arrays concatenated in rank order."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dist_gfa_model as dm
import gfa_model
from helpers import pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


# ---- 1. the numbered writer on hand-made arrays ------------------------------------------------------------------------------
K5 = 5
LENGTHS = [5, 6, 7, 9, 13, 16, 17, 21, 32, 33, 48, 70]      # 16-byte stores straddle names, tags, newlines and segment ends
FIRSTS = [0, 7, 95, 999999990, 2 ** 32 - 3, 10 ** 19]        # 9 -> 10, 99 -> 100, 10^9 -> 10^10 digits; the u32 wrap; 20 digits


def _u64_tensor(values):
    return torch.from_numpy(np.array(values, np.uint64).view(np.int64).copy()).cuda()


def _device_part(k, weight, seqs, off=None, shift=0):
    """-> (edge_weight, edge_kmers, edge_label_off, edge_label, label_bytes) on the device; shift: bytes in front of the labels"""
    raw = [gfa_model.compress_edge(s) for s in seqs]
    if off is None:
        off = np.zeros(len(raw) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in raw])
    blob = b"\0" * shift + b"".join(raw)
    lab = torch.from_numpy(np.frombuffer(blob + b"\0" * (16 + -len(blob) % 4), np.uint8).copy()).cuda()[shift:]
    kmers = [len(s) - k + 1 for s in seqs]
    u32 = lambda a: torch.from_numpy(np.array(a, np.uint32).view(np.int32).copy()).cuda()
    return u32(weight), u32(kmers), torch.from_numpy(np.asarray(off, np.int64)).cuda(), lab, len(blob) - shift


def _check_part(k, weight, seqs, first, with_header, link_first, link_b):
    """the part on the device against the model: S part, L part, segment_off, the sizes and the zero padding, byte for byte"""
    from katome_amd import device as kd
    w, km, off, lab, label_bytes = _device_part(k, weight, seqs)
    text, s_bytes, l_offset, l_bytes, seg = kd.gfa_part_arrays(k, w, km, off, lab, first, with_header, _u64_tensor(link_first), _u64_tensor(link_b),
                                                               label_bytes=label_bytes)
    kmers = [len(s) - k + 1 for s in seqs]
    s_want, l_want, seg_want = dm.part_text(k, weight, kmers, seqs, first, with_header, link_first, link_b)
    assert (s_bytes, l_bytes, l_offset) == (len(s_want), len(l_want), len(dm.padded(s_want)))
    got = bytes(text.cpu().numpy())
    assert len(got) == len(dm.padded(s_want)) + len(dm.padded(l_want))
    assert got[:l_offset] == dm.padded(s_want)
    assert got[l_offset:] == dm.padded(l_want)
    assert seg.cpu().tolist() == seg_want
    return s_want, l_want


@pytest.fixture(scope="module")
def hand_made():
    rng = np.random.default_rng(12)
    seqs = ["".join(rng.choice(list("ACGT"), n)) for n in LENGTHS]
    # KC = weight * k-mers: both factors are 32-bit and a label's k-mers stay below 2^31, so KC stays below 2^63 (19 digits); with
    # these lengths the largest is (2^32 - 1) * 66, 12 digits, next to products of 1, 2 and 10 digits
    weight = [1, 9, 10, 2 ** 32 - 1, 99999, 1, 2 ** 31, 7, 2 ** 32 - 1, 1000000, 3, 2 ** 32 - 1]
    assert len(str(weight[-1] * (LENGTHS[-1] - K5 + 1))) == 12
    return seqs, weight


def _hand_links(first):
    """a link table whose b values cross the digit boundaries of FIRSTS, 20 digits and 2^64 - 1 included; segments with 0 .. 4 links"""
    counts = [0, 1, 2, 4, 0, 3, 1, 1, 0, 4, 2, 1]
    pool = [0, 9, 10, 99, 100, 999999999, 10 ** 9, 2 ** 32 - 1, 2 ** 32, 10 ** 19 - 1, 10 ** 19, 2 ** 64 - 1, first, first + 11, 7, 95, 5, 12345678901234, 42]
    link_first = [0] + list(np.cumsum(counts))
    link_b = [pool[i % len(pool)] for i in range(link_first[-1])]
    return [int(x) for x in link_first], link_b


@pytest.mark.parametrize("with_header", [0, 1])
@pytest.mark.parametrize("first", FIRSTS)
def test_numbered_part(hand_made, first, with_header):
    seqs, weight = hand_made
    link_first, link_b = _hand_links(first)
    s, l = _check_part(K5, weight, seqs, first, with_header, link_first, link_b)
    assert s.startswith(dm.HEADER) == bool(with_header)
    assert (b"S\t%d\t" % (first + 11)) in s and (b"L\t%d\t+\t%d\t+\t4M\n" % (first + 1, link_b[0])) in l


def test_parts_of_more_than_two_tiles(hand_made):
    """S part and L part of more than two 8192-byte tiles each, with a line of 20-digit numbers lying across a tile boundary in both"""
    rng = np.random.default_rng(5)
    first = 10 ** 19
    n = 400
    lengths = [LENGTHS[i % len(LENGTHS)] for i in range(n)]
    lengths[0] = 3000                                        # (KC of 14 digits; the 16-base stores run through a long segment)
    seqs = ["".join(rng.choice(list("ACGT"), m)) for m in lengths]
    weight = [2 ** 32 - 1] + [int(x) for x in rng.integers(1, 2 ** 32, n - 1)]
    link_first = list(range(n + 1))                          # one link each: L lines of 51 bytes, so line 160 lies across byte 8192
    link_b = [first + int(x) for x in rng.integers(0, n, n)]
    s, l = _check_part(K5, weight, seqs, first, 1, link_first, link_b)
    assert len(s) > 2 * dm.TILE and len(l) > 2 * dm.TILE
    assert dm.lines_across_tiles(s, 20) and dm.lines_across_tiles(l, 20)
    assert len(str(weight[0] * (3000 - K5 + 1))) == 14


def test_from_zero_with_header_is_the_one_gpu_text(hand_made):
    """first_segment = 0, with_header = 1 and the link table of katome_dev_gfa_arrays: the parts put together are that entry's text"""
    from katome_amd import device as kd
    seqs, weight = hand_made
    rng = np.random.default_rng(3)
    n, n_nodes = len(seqs), 4
    src, dst = [int(x) for x in rng.integers(0, n_nodes, n)], [int(x) for x in rng.integers(0, n_nodes, n)]
    w, km, off, lab, label_bytes = _device_part(K5, weight, seqs)
    i64 = lambda a: torch.from_numpy(np.array(a, np.int64)).cuda()
    g = kd.gfa_arrays(K5, n_nodes, i64(src), i64(dst), w, km, off, lab, label_bytes=label_bytes)
    link_first, link_b = dm.link_table(src, dst)
    assert g.link_first.cpu().tolist() == link_first and g.n_links == len(link_b) > 0
    text, s_bytes, l_offset, l_bytes, seg = kd.gfa_part_arrays(K5, w, km, off, lab, 0, 1, g.link_first, _u64_tensor(link_b), label_bytes=label_bytes)
    got = bytes(text.cpu().numpy())
    one = bytes(g.text.cpu().numpy())
    assert got[:s_bytes] + got[l_offset:l_offset + l_bytes] == one == gfa_model.gfa_text(K5, src, dst, weight, [len(s) - K5 + 1 for s in seqs], seqs)[0]
    assert torch.equal(seg, g.segment_off)


def test_part_refusals(hand_made):
    from katome_amd import _lib, device as kd
    from katome_amd.build import KatomePanic
    seqs, weight = hand_made
    n = len(seqs)
    link_first, link_b = _hand_links(0)
    w, km, off, lab, label_bytes = _device_part(K5, weight, seqs)

    def refused(name, first=0, lf=link_first, lab_=lab, off_=off, nbytes=label_bytes):
        with pytest.raises(KatomePanic) as e:
            kd.gfa_part_arrays(K5, w, km, off_, lab_, first, 1, _u64_tensor(lf), _u64_tensor(link_b), label_bytes=nbytes)
        assert e.value.name == name, e.value
        return e.value.message

    assert "2^64" in refused("E_UNSUPPORTED", first=2 ** 64 - n + 1)                 # first_segment + n_edges past 2^64
    kd.gfa_part_arrays(K5, w, km, off, lab, 2 ** 64 - 1 - n, 1, _u64_tensor(link_first), _u64_tensor(link_b), label_bytes=label_bytes)      # the last that fits
    down = list(link_first)
    down[5], down[6] = down[6], down[5] - 1
    assert "ascend" in refused("E_ARG", lf=down)                                      # a d_link_first that does not ascend
    assert "ascend" in refused("E_ARG", lf=[1] + link_first[1:])                      # ... or does not start at 0
    w1, km1, off1, lab1, nb1 = _device_part(K5, weight, seqs, shift=1)
    assert "aligned" in refused("E_ARG", lab_=lab1, off_=off1, nbytes=nb1)           # a misaligned label pointer
    bad = off.clone()
    bad[3] = bad[4]
    assert "label" in refused("E_ARG", off_=bad)                                      # malformed labels, before anything is read through them
    # a size query: d_text NULL sets the three sizes and writes nothing
    sb, lo, lb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lf_t, lb_t = _u64_tensor(link_first), _u64_tensor(link_b)
    assert _lib.lib().katome_dev_gfa_part_arrays(0, K5, n, w.data_ptr(), km.data_ptr(), off.data_ptr(), lab.data_ptr(), label_bytes, 95, 0, lf_t.data_ptr(),
                                                 lb_t.data_ptr(), None, None, 0, C.byref(sb), C.byref(lo), C.byref(lb), None) == 0
    s_want, l_want, _ = dm.part_text(K5, weight, [len(s) - K5 + 1 for s in seqs], seqs, 95, False, link_first, link_b)
    assert (sb.value, lo.value, lb.value) == (len(s_want), len(dm.padded(s_want)), len(l_want))
    # ... and a buffer that is too small is refused
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    seg = torch.zeros(n, dtype=torch.int64, device="cuda")
    assert _lib.lib().katome_dev_gfa_part_arrays(0, K5, n, w.data_ptr(), km.data_ptr(), off.data_ptr(), lab.data_ptr(), label_bytes, 95, 0, lf_t.data_ptr(),
                                                 lb_t.data_ptr(), seg.data_ptr(), small.data_ptr(), 64, C.byref(sb), C.byref(lo), C.byref(lb), None) != 0


# ---- what a GFA text says, by sequence ----------------------------------------------------------------------------------------
def _graph_of(data, k):
    """a GFA file of this library -> (segments as a sorted list of (sequence, LN, KC, ew), links as a sorted list of pairs of
    sequences, the parsed segments, the parsed links); names count up from 0, links come by a, then b, every overlap is k - 1"""
    segments, lks = gfa_model.parse(data)
    assert [s[0] for s in segments] == list(range(len(segments)))
    assert [(a, b) for a, b, _ in lks] == sorted((a, b) for a, b, _ in lks) and all(o == k - 1 for _, _, o in lks)
    assert all(t["LN"] == len(seq) and t["KC"] == t["ew"] * (len(seq) - k + 1) for _, seq, t in segments)
    seqs = [s[1] for s in segments]
    assert len(set(seqs)) == len(seqs)                                   # every k-mer lies on one edge: unitig sequences are distinct
    return (sorted((seq, t["LN"], t["KC"], t["ew"]) for _, seq, t in segments), sorted((seqs[a], seqs[b]) for a, b, _ in lks), segments, lks)


def _links_by_overlap(seqs, k):
    """gfa_model.links with a segment's two vertices read off its sequence: its first and its last k - 1 bases"""
    ids = {}
    src = [ids.setdefault(s[:k - 1], len(ids)) for s in seqs]
    dst = [ids.setdefault(s[len(s) - k + 1:], len(ids)) for s in seqs]
    return sorted((seqs[a], seqs[b]) for a, b in gfa_model.links(src, dst))


# ---- 2. process ranks ----------------------------------------------------------------------------------------------------------
def _clean(ascii_reads):
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    return clean


def _input(k):
    """the shapes of test_gpu_dist_text.py"""
    return (3000, 200, 30000, 1e-3) if k > 40 else (2500, 110, 50000, 8e-3)


THR, GLEN = 2, 3000


def _one_gpu(packed, n, L, k, rc, first_seen, chain):
    from katome_amd import device as kd
    b = kd.Builder(k, rc, first_seen_order=first_seen)
    p = torch.from_numpy(np.concatenate([packed, np.zeros(32, np.uint8)])).cuda()
    span = b.tile_span(L)
    if span > 1:
        b.insert_tiles(b.extract_tiles(p, n, L, span), span)
    else:
        b.insert(b.extract_fixed(p, n, L))
    b.finalize()
    for st in chain:
        {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.remove_weak_edges(THR), "e": lambda: b.standardize_edges(GLEN, THR)}[st]()
    return b, b.shrink(mode="fast")


def _process_rank(rank, world, k, rc, first_seen, chain, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    import torch.distributed as dist
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    # (the ranks meet through a file: a port picked in advance can be taken by another process before rank 0 listens on it)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = ks.Comm.over_torch(device=0)
        from oracle import oracle as o
        n, L, G, err = _input(k)
        reads = _clean(o.synth_reads(0, n, L, G, err, 1))
        first, count = ks.shard_range(len(reads), world, rank)
        packed = torch.from_numpy(np.concatenate([pack_reads_ascii(reads[first:first + count]).reshape(-1), np.zeros(32, np.uint8)])).cuda()
        b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=first_seen)
        try:
            b.contigs_gfa()
            raise AssertionError("a GFA without a shrink")
        except KatomePanic as e:
            assert e.name == "E_ARG", e
        b.add_reads(packed, first, count, L, None, batch_reads=1024)
        b.finalize()
        for st in chain:
            {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.prune_weak_edges(THR), "e": lambda: b.standardize_edges(GLEN, THR)}[st]()
        c = b.shrink()
        u = lambda t, dt: t.cpu().numpy().view(dt).copy()
        h = dict(seqs=np.array(c.sequences(), dtype=object), src=u(c.edge_src, np.uint64), dst=u(c.edge_dst, np.uint64),
                 weight=u(c.edge_weight, np.uint32), kmers=u(c.edge_kmers, np.uint32), total_nodes=np.array([c.total_nodes], np.uint64))
        g = b.contigs_gfa()
        h["s_text"], h["l_text"] = u(g.s_text, np.uint8), u(g.l_text, np.uint8)
        h["segment_off"], h["link_first"], h["link_b"] = u(g.segment_off, np.int64), u(g.link_first, np.int64), u(g.link_b, np.uint64)
        h["counts"] = np.array([g.n_segments, g.first_segment, g.total_segments, g.n_links, g.total_links, g.s_bytes, g.s_base, g.l_bytes, g.l_base,
                                g.total_text_bytes], np.uint64)
        b.save_gfa(g, os.path.join(out_dir, "all.gfa"))            # (process ranks on one filesystem)
        a = b.contigs_text("fasta")
        h["fasta"] = u(a.text, np.uint8)
        c2 = b.shrink()                                             # a second shrink makes the GFA stale for the save
        try:
            b.save_gfa(g, os.path.join(out_dir, "stale.gfa"))
            raise AssertionError("a stale GFA was saved")
        except KatomePanic as e:
            assert e.name == "E_ARG", e
        del a, c, c2, g
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **h)
        b.close()
        comm.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,k,rc,first_seen,chain", [(3, 31, True, True, "dcwced"), (4, 63, False, False, ""), (1, 31, True, True, ""),
                                                                 (1, 31, True, False, "")])
def test_process_ranks(oracle, tmp_path, world, k, rc, first_seen, chain):
    import torch.multiprocessing as mp
    mp.spawn(_process_rank, args=(world, k, rc, first_seen, chain, str(tmp_path)), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r), allow_pickle=True) for r in range(world)]
    assert not os.path.exists(os.path.join(str(tmp_path), "stale.gfa"))
    counts, n_links = [len(p["seqs"]) for p in parts], [len(p["link_b"]) for p in parts]
    s_sizes, l_sizes = [len(p["s_text"]) for p in parts], [len(p["l_text"]) for p in parts]
    assert sum(counts) > 10 and sum(n_links) > 10
    # the counts and the bases add up across ranks
    for r, p in enumerate(parts):
        ns, first, total, nl, tl, sb, s_base, lb, l_base, tb = (int(x) for x in p["counts"])
        assert (ns, first, total) == (counts[r], sum(counts[:r]), sum(counts))
        assert (nl, tl) == (n_links[r], sum(n_links))
        assert (sb, s_base, lb, l_base, tb) == (s_sizes[r], sum(s_sizes[:r]), l_sizes[r], sum(s_sizes) + sum(l_sizes[:r]), sum(s_sizes) + sum(l_sizes))
    # header + S parts + L parts: gfa_text of the concatenated arrays, byte for byte, and the saved file
    cat = lambda name: np.concatenate([p[name] for p in parts])
    seqs = cat("seqs").tolist()
    want, seg_want, first_want = gfa_model.gfa_text(k, cat("src"), cat("dst"), cat("weight"), cat("kmers"), seqs)
    whole = b"".join(bytes(p["s_text"]) for p in parts) + b"".join(bytes(p["l_text"]) for p in parts)
    assert whole[:11] == dm.HEADER and whole == want
    assert open(os.path.join(str(tmp_path), "all.gfa"), "rb").read() == whole
    # segment_off and link_first index what they claim; segment i carries the sequence of the sharded FASTA record >katome_<i>
    ab = gfa_model.links(cat("src"), cat("dst"))
    fasta = b"".join(bytes(p["fasta"]) for p in parts).decode().split("\n")
    assert fasta[0:-1:2] == [">katome_%d" % i for i in range(sum(counts))] and fasta[1:-1:2] == seqs
    at = 0
    for r, p in enumerate(parts):
        first, s_text = sum(counts[:r]), bytes(p["s_text"])
        assert [s_text[o:o + len(s)].decode() for o, s in zip(p["segment_off"].tolist(), p["seqs"].tolist())] == p["seqs"].tolist()
        assert [s_text[o - 3 - len(str(first + j)):o].decode() for j, o in enumerate(p["segment_off"].tolist())] == ["S\t%d\t" % (first + j) for j in range(counts[r])]
        lf = p["link_first"].tolist()
        assert lf[0] == 0 and lf[-1] == n_links[r] and lf == [x - first_want[first] for x in first_want[first:first + counts[r] + 1]]
        lines = bytes(p["l_text"]).decode().split("\n")[:-1]
        assert len(lines) == n_links[r]
        for j in range(counts[r]):
            assert [(first + j, int(b)) for b in p["link_b"][lf[j]:lf[j + 1]]] == ab[at:at + lf[j + 1] - lf[j]]
            assert all(ln.startswith("L\t%d\t+\t" % (first + j)) for ln in lines[lf[j]:lf[j + 1]])
            at += lf[j + 1] - lf[j]
    assert at == len(ab)
    got_segments, got_links, _, _ = _graph_of(whole, k)
    assert got_links == _links_by_overlap(seqs, k)
    if first_seen or world == 1:
        n, L, G, err = _input(k)
        packed = pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy()
        if world == 1 and not first_seen:
            # one rank, by packed key: the file of the one-GPU host entry
            from katome_amd.build import GpuGraph
            one = GpuGraph.gfa_from_packed(packed, n, L, reverse_complement=rc, stages="", k=k, first_seen_order=False)
            assert bytes(np.ctypeslib.as_array(one._gp.contents.text, (one._gp.contents.text_bytes,))) == whole
            del one
        b, dc = _one_gpu(packed, n, L, k, rc, first_seen, chain)
        ref = dc.gfa()
        ref_segments, ref_links, _, _ = _graph_of(ref.bytes(), k)
        assert got_segments == ref_segments and got_links == ref_links
        del ref, dc
        b.close()


# ---- 3. the host entry on thread ranks ---------------------------------------------------------------------------------------
K, RC = 31, True
_cache = {}


def _reads(oracle):
    if "reads" not in _cache:
        n, L, G, err = _input(K)
        _cache["reads"] = (pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy(), n, L)
    return _cache["reads"]


def _gfa(oracle, tmp_path, n_devices, stages, name="u.gfa", first_seen=True, **kw):
    from katome_amd.build import GpuUnitigs
    packed, n, L = _reads(oracle)
    out = str(tmp_path / name)
    u, _ = GpuUnitigs.gfa_from_packed(packed, n, L, reverse_complement=RC, minimal_weight_threshold=THR, output_file=out, stages=stages,
                                      original_genome_length=GLEN, k=K, first_seen_order=first_seen, n_devices=n_devices,
                                      ranks_share_device=n_devices > 1, **kw)
    return u, open(out, "rb").read()


def _numbers(u):
    return (u.n_segments, u.n_links, u.total_bases, u.longest, u.read_bytes, u.k)


def _one_device(oracle, tmp_path, stages):
    if stages not in _cache:
        u, data = _gfa(oracle, tmp_path, 1, stages, "one_%s.gfa" % stages)
        assert u.n_devices == 1 and u.n_segments > 10 and u.n_links > 10 and u.shrink["rank_rounds"] == 0 and u.text_bytes == len(data)
        _cache[stages] = (_numbers(u), data, _graph_of(data, K)[:2])
    return _cache[stages]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("stages", ["", "dcwced"])
def test_one_device_file_is_the_device_text(oracle, tmp_path, stages):
    numbers, data, (segments, lks) = _one_device(oracle, tmp_path, stages)
    packed, n, L = _reads(oracle)
    b, dc = _one_gpu(packed, n, L, K, RC, True, stages)
    g = dc.gfa()
    assert data == g.bytes()
    seqs = dc.sequences()
    assert numbers == (len(seqs), g.n_links, sum(map(len, seqs)), max(map(len, seqs)), n * L, K)
    assert lks == _links_by_overlap(seqs, K)
    del g, dc
    b.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("stages", ["", "dcwced"])
@pytest.mark.parametrize("n_devices", [2, 3, 8])
def test_thread_ranks_equal_one_device(oracle, tmp_path, n_devices, stages):
    want, _, want_graph = _one_device(oracle, tmp_path, stages)
    u, data = _gfa(oracle, tmp_path, n_devices, stages)
    assert u.n_devices == n_devices and len(data) == u.text_bytes
    assert _graph_of(data, K)[:2] == want_graph
    assert _numbers(u) == want
    assert u.shrink["longest_path"] + K - 1 == u.longest and u.shrink["rank_rounds"] > 0


@pytest.mark.timeout(300)
def test_small_chunks_write_the_same_bytes(oracle, tmp_path, monkeypatch):
    _, whole = _gfa(oracle, tmp_path, 3, "dcwced", "whole.gfa")
    monkeypatch.setenv("KATOME_DIST_GFA_CHUNK", "50")
    monkeypatch.setenv("KATOME_DIST_TEXT_CHUNK", "1000")
    _, chunked = _gfa(oracle, tmp_path, 3, "dcwced", "chunked.gfa")
    assert chunked == whole and len(whole) > 5000


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures(golden_dir, tmp_path, i):
    """tests/shrinker.rs:33-36: 1, 92 and 233 merged edges, in both numberings, on 3 ranks"""
    from katome_amd.build import GpuUnitigs, InputFileType, set_global_k_sizes
    pinned = json.load(open(os.path.join(golden_dir, "pinned.json")))
    k = pinned["k"]
    set_global_k_sizes(k)
    out = str(tmp_path / "f.gfa")
    path = [os.path.join(golden_dir, pinned["fixtures"][i])]
    one, _ = GpuUnitigs.gfa(path, InputFileType.Fastq, False, output_file=out, original_genome_length=100, first_seen_order=True)
    one_segments, one_links, parsed, _ = _graph_of(open(out, "rb").read(), k)
    assert one.n_segments == pinned["shrink"]["counts"][i][1]
    assert one_links == _links_by_overlap([s[1] for s in parsed], k) and len(one_links) == one.n_links
    for first_seen in (True, False):
        u, read_bytes = GpuUnitigs.gfa(path, InputFileType.Fastq, False, output_file=out, original_genome_length=100, first_seen_order=first_seen,
                                       n_devices=3, ranks_share_device=True)
        assert u.n_segments == pinned["shrink"]["counts"][i][1] and read_bytes == pinned["read_bytes"]["values"][i]
        segments, lks, _, _ = _graph_of(open(out, "rb").read(), k)
        assert segments == one_segments and lks == one_links and u.n_links == len(lks)


# ---- 4. edge cases of the join ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_one_read_on_eight_ranks(oracle, tmp_path):
    """one read of four 31-mers, by packed key: one segment, no link; most ranks hold no edge and write nothing"""
    from katome_amd.build import GpuUnitigs
    L = 34
    reads = oracle.synth_reads(3, 1, L, 5000, 0.0, 0)
    out = str(tmp_path / "one.gfa")
    u, _ = GpuUnitigs.gfa_from_packed(pack_reads_ascii(reads).reshape(-1).copy(), 1, L, k=31, output_file=out, original_genome_length=34,
                                      n_devices=8, ranks_share_device=True)
    seq = reads[0].tobytes().decode()
    assert open(out, "rb").read().decode() == "H\tVN:Z:1.0\nS\t0\t%s\tLN:i:34\tKC:i:4\tew:i:1\n" % seq
    assert (u.n_segments, u.n_links, u.total_bases, u.longest) == (1, 0, 34, 34)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_devices", [1, 2])
def test_no_edges_at_all(oracle, tmp_path, n_devices):
    """every read is skipped: the header line alone"""
    from katome_amd.build import GpuUnitigs
    packed, n, L = _reads(oracle)
    out = str(tmp_path / "empty.gfa")
    u, read_bytes = GpuUnitigs.gfa_from_packed(packed[:64 * ((L + 3) // 4)], 64, L, skip=np.ones(64, np.uint8), k=K, output_file=out,
                                               original_genome_length=1000, n_devices=n_devices, ranks_share_device=n_devices > 1)
    assert open(out, "rb").read() == dm.HEADER and read_bytes == 0
    assert (u.n_segments, u.n_links, u.text_bytes, u.total_bases, u.longest) == (0, 0, 11, 0, 0)


def _circle(k, n, seed):
    """a circular sequence of n bases without a repeated (k - 1)-mer"""
    rng = np.random.default_rng(seed)
    while True:
        s = "".join(rng.choice(list("ACGT"), n))
        ring = s + s[:k - 2]
        if len({ring[i:i + k - 1] for i in range(n)}) == n:
            return s


@pytest.mark.timeout(300)
def test_a_cycle_is_one_segment_linked_to_itself(oracle, tmp_path):
    """a circular sequence read in overlapping windows shrinks to one edge (checked with the oracle on the CPU): the cycle's
    self-loop is one segment linked to itself, on 3 ranks"""
    from katome_amd.build import GpuUnitigs
    k, n, L = 31, 120, 60
    ring = _circle(k, n, 1)
    reads = np.array([list((ring + ring)[i:i + L].encode()) for i in range(0, n, 20)], np.uint8)       # windows that overlap by 40 > k
    edges = {}
    for r in reads:
        s = r.tobytes().decode()
        for j in range(L - k + 1):
            edges[s[j:j + k]] = edges.get(s[j:j + k], 0) + 1
    assert len(edges) == n                                         # every k-mer of the ring, none else: n vertices of in- and out-degree 1
    src, dst = [e[:-1] for e in edges], [e[1:] for e in edges]
    assert sorted(src) == sorted(dst) and len(set(src)) == n
    out = str(tmp_path / "ring.gfa")
    u, _ = GpuUnitigs.gfa_from_packed(pack_reads_ascii(reads).reshape(-1).copy(), len(reads), L, k=k, output_file=out, original_genome_length=n,
                                      first_seen_order=True, n_devices=3, ranks_share_device=True)
    segments, lks, parsed, parsed_links = _graph_of(open(out, "rb").read(), k)
    assert (u.n_segments, u.n_links) == (1, 1) and [(a, b) for a, b, _ in parsed_links] == [(0, 0)]
    seq = parsed[0][1]
    assert len(seq) == n + k - 1 and seq[:k - 1] == seq[n:] and seq[:n] in ring + ring
    assert u.shrink["cycles"] == 1


@pytest.mark.timeout(300)
def test_four_out_segments_and_none(oracle, tmp_path):
    """a vertex with four out-segments and segments without any: both asserted from the parsed result"""
    from katome_amd.build import GpuUnitigs
    k, L = 31, 50
    rng = np.random.default_rng(9)
    stem = "".join(rng.choice(list("ACGT"), 35))
    tails = ["".join(rng.choice(list("ACGT"), 14)) for _ in range(4)]
    reads = np.array([list((stem + c + t).encode()) for c, t in zip("ACGT", tails)], np.uint8)         # one stem, then the four bases
    assert reads.shape == (4, L)
    out = str(tmp_path / "fork.gfa")
    for n_devices, first_seen in ((3, True), (8, False)):
        u, _ = GpuUnitigs.gfa_from_packed(pack_reads_ascii(reads).reshape(-1).copy(), 4, L, k=k, output_file=out, original_genome_length=100,
                                          first_seen_order=first_seen, n_devices=n_devices, ranks_share_device=True)
        segments, lks, parsed, parsed_links = _graph_of(open(out, "rb").read(), k)
        outs = {}
        for a, b, _ in parsed_links:
            outs.setdefault(a, []).append(b)
        assert (u.n_segments, u.n_links) == (5, 4)
        assert sorted(len(v) for v in outs.values()) == [4]          # the stem's end has four out-segments ...
        assert sum(1 for s in parsed if s[0] not in outs) == 4        # ... and the four tails have none
        assert lks == _links_by_overlap([s[1] for s in parsed], k)


# ---- 5. failures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_failure_reaches_every_rank(oracle, tmp_path, monkeypatch):
    """KATOME_DIST_GFA_FAIL=1 on four ranks: the call returns rank 1's failure, no file is left behind; a clean run follows"""
    from katome_amd.build import KatomePanic
    monkeypatch.setenv("KATOME_DIST_GFA_FAIL", "1")
    with pytest.raises(KatomePanic) as e:
        _gfa(oracle, tmp_path, 4, "", "fail.gfa")
    assert e.value.name == "E_UNSUPPORTED" and "rank 1" in e.value.message
    assert not os.path.exists(str(tmp_path / "fail.gfa"))
    monkeypatch.delenv("KATOME_DIST_GFA_FAIL")
    u, data = _gfa(oracle, tmp_path, 4, "", "fail.gfa")
    assert u.n_segments > 10 and len(data) == u.text_bytes


@pytest.mark.timeout(300)
def test_refusals(oracle, tmp_path):
    from katome_amd.build import KatomePanic
    for n_devices in (1, 3):
        bad = tmp_path / "no_such_dir" / "u.gfa"
        with pytest.raises(KatomePanic) as e:                                             # asm/mod.rs:62
            _gfa(oracle, tmp_path, n_devices, "", os.path.join("no_such_dir", "u.gfa"))
        assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
        with pytest.raises(KatomePanic) as e:                                             # stage letters on a by-key build
            _gfa(oracle, tmp_path, n_devices, "dcwced", first_seen=False)
        assert e.value.name == "E_ARG" and "FIRST_SEEN" in e.value.message
    u, data = _gfa(oracle, tmp_path, 3, "", "by_key.gfa", first_seen=False)               # a packed-key build without them is fine
    assert _graph_of(data, K)[:2] == _one_device(oracle, tmp_path, "")[2]
