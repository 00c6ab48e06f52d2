"""The end of the sharded pipeline (katome_amd/csrc/dist_text.hip; collapse.hip's text kernel with a starting number): contig
numbers that start anywhere, the text and Contigs::stats of the sharded shrink on process ranks, the stats of sharded lists against
the host function, and the host entry katome_unitigs_* on thread ranks -- its file, its numbers, its failures."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from helpers import pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


# ---- contig numbers that start anywhere ------------------------------------------------------------------------------------
K5 = 5
LENGTHS = [5, 6, 7, 9, 13, 16, 17, 21, 32, 33, 48, 70]      # 16-byte stores straddle headers, newlines and contig ends
FIRSTS = [0, 7, 95, 999999990, 2 ** 32 - 3, 10 ** 19]        # 9 -> 10, 99 -> 100, 10^9 -> 10^10 digits; the u32 wrap; 20 digits


def compress_edge(seq):
    """compress.rs:250-271"""
    pad = (4 - len(seq) % 4) % 4
    codes = ["ACGT".index(c) for c in seq] + [0] * pad
    return bytes([pad] + [codes[i] << 6 | codes[i + 1] << 4 | codes[i + 2] << 2 | codes[i + 3] for i in range(0, len(codes), 4)])


@pytest.fixture(scope="module")
def hand_made():
    rng = np.random.default_rng(12)
    contigs = ["".join(rng.choice(list("ACGT"), n)) for n in LENGTHS]
    raw = [compress_edge(s) for s in contigs]
    off = np.zeros(len(raw) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raw])
    lab = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, np.uint8).copy()).cuda()
    return contigs, lab, torch.from_numpy(off).cuda()


def encoded(contigs, layout, first):
    return "".join(contigs) if layout == "plain" else "".join(">katome_%d\n%s\n" % (first + i, c) for i, c in enumerate(contigs))


@pytest.mark.parametrize("layout", ["plain", "fasta"])
@pytest.mark.parametrize("first", FIRSTS)
def test_numbering(hand_made, layout, first):
    from katome_amd import device as kd
    contigs, lab, off = hand_made
    c_off, c_len, text, n = kd.pieces_text(lab, off, None, K5, layout, first_contig=first)
    text = bytes(text.cpu().numpy()[:n]).decode()
    assert text == encoded(contigs, layout, first)
    assert [text[o:o + ln] for o, ln in zip(c_off.cpu().tolist(), c_len.cpu().tolist())] == contigs


@pytest.mark.parametrize("layout", ["plain", "fasta"])
def test_numbering_from_zero_is_the_old_entry(hand_made, layout):
    from katome_amd import _lib, device as kd
    contigs, lab, off = hand_made
    L = _lib.lib()
    nc, nb = C.c_uint64(), C.c_uint64()
    c_off = torch.empty(len(contigs), dtype=torch.int64, device="cuda")
    c_len = torch.empty(len(contigs), dtype=torch.int32, device="cuda")
    text = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert L.katome_dev_pieces_text(0, K5, lab.data_ptr(), off.data_ptr(), len(contigs), None, len(contigs), kd.LAYOUTS[layout], c_off.data_ptr(),
                                    c_len.data_ptr(), len(contigs), text.data_ptr(), 4096, C.byref(nc), C.byref(nb), None) == 0
    new_off, new_len, new_text, n = kd.pieces_text(lab, off, None, K5, layout, first_contig=0)
    assert (nc.value, nb.value) == (len(contigs), n)
    assert bytes(text.cpu().numpy()[:n]) == bytes(new_text.cpu().numpy()[:n]) == encoded(contigs, layout, 0).encode()
    assert torch.equal(c_off, new_off) and torch.equal(c_len, new_len)


def test_numbers_past_64_bits_are_refused(hand_made):
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    contigs, lab, off = hand_made
    with pytest.raises(KatomePanic) as e:
        kd.pieces_text(lab, off, None, K5, "fasta", first_contig=2 ** 64 - 5)
    assert e.value.name == "E_UNSUPPORTED"
    # the last number that fits
    _, _, text, n = kd.pieces_text(lab, off, None, K5, "fasta", first_contig=2 ** 64 - 1 - len(contigs))
    assert bytes(text.cpu().numpy()[:n]).decode() == encoded(contigs, "fasta", 2 ** 64 - 1 - len(contigs))


# ---- process ranks -----------------------------------------------------------------------------------------------------------
def _clean(ascii_reads):
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    return clean


def _input(k):
    """the shapes of test_gpu_dist_shrink.py"""
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


def _stats_cases(rank, world, case):
    """seeded lists with ties, giants and empty ranks -> (this rank's k-mer counts, all of them, k, genome length)"""
    rng = np.random.default_rng(1000 + case)
    n = int(rng.choice([0, 1, 2, 7, 300, 5000]))
    top = int(rng.choice([2, 3, 50, 70000, 2 ** 32]))
    m = rng.integers(1, top, n, dtype=np.uint64).astype(np.uint32)
    if n and case % 3 == 0:
        m[int(rng.integers(0, n))] = 2 ** 32 - 1
    if n and case % 5 == 0:
        m[:] = m[0]
    owners = np.arange(world) if case % 2 else rng.choice(world, size=max(1, world // 2), replace=False)
    who = rng.choice(owners, size=n) if n else np.zeros(0, np.int64)
    k = int(rng.choice([3, 5, 31, 63]))
    total = int(m.astype(np.uint64).sum()) + n * (k - 1)
    genome = [0, 1, 2, total, 3 * total, int(rng.integers(0, 2 * total + 3))][case % 6]
    return m[who == rank], m, k, genome


def _process_rank(rank, world, mode, k, rc, first_seen, chain, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    import torch.distributed as dist
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic, contig_stats
    # (the ranks meet through a file: a port picked in advance can be taken by another process before rank 0 listens on it)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = ks.Comm.over_torch(device=0)
        if mode == "stats":
            for case in range(36):
                mine, every, kk, genome = _stats_cases(rank, world, case)
                d_mine = torch.from_numpy(mine.view(np.int32).copy()).cuda()
                lengths = every.astype(np.uint64) + np.uint64(kk - 1)
                try:
                    want = contig_stats(lengths, genome).astuple()
                except KatomePanic as e:
                    want = (e.name, e.message)
                try:
                    got = ks.contig_stats_arrays(comm, d_mine, kk, genome).astuple()
                except KatomePanic as e:
                    got = (e.name, e.message)
                assert got == want, (case, got, want)
            np.savez(os.path.join(out_dir, "rank%d.npz" % rank), ok=np.ones(1))
            comm.close()
            return
        from oracle import oracle as o
        n, L, G, err = _input(k)
        reads = _clean(o.synth_reads(0, n, L, G, err, 1))
        first, count = ks.shard_range(len(reads), world, rank)
        packed = torch.from_numpy(np.concatenate([pack_reads_ascii(reads[first:first + count]).reshape(-1), np.zeros(32, np.uint8)])).cuda()
        b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=first_seen)
        try:
            b.contigs_text("fasta")
            raise AssertionError("text without a shrink")
        except KatomePanic as e:
            assert e.name == "E_ARG", e
        b.add_reads(packed, first, count, L, None, batch_reads=1024)
        b.finalize()
        for st in chain:
            {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.prune_weak_edges(THR), "e": lambda: b.standardize_edges(GLEN, THR)}[st]()
        c = b.shrink()
        h = dict(seqs=np.array(c.sequences(), dtype=object), head=c.edge_head_id.cpu().numpy(), kmers=c.edge_kmers.cpu().numpy().view(np.uint32))
        for layout in ("plain", "fasta"):
            a = b.contigs_text(layout)
            h[layout] = a.text.cpu().numpy().copy()
            h[layout + "_off"], h[layout + "_len"] = a.contig_off.cpu().numpy(), a.contig_len.cpu().numpy()
            h[layout + "_counts"] = np.array([a.n_contigs, a.first_contig, a.total_contigs, a.text_bytes, a.text_base, a.total_text_bytes], np.uint64)
            assert a.layout == layout
        b.save_contigs(a, os.path.join(out_dir, "all.fa"))       # (the FASTA text: process ranks on one filesystem)
        h["stats"] = np.array(b.contig_stats(GLEN).astuple(), np.uint64)
        try:
            b.contig_stats(1)
            raise AssertionError("a tipping point of 0 went through")
        except KatomePanic as e:
            assert e.name == "E_ARG" and "ng50" in e.message, e
        del a, c
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **h)
        b.close()
        comm.close()
    finally:
        dist.destroy_process_group()


def _spawn(world, *args):
    import torch.multiprocessing as mp
    mp.spawn(_process_rank, args=(world,) + args, nprocs=world, join=True)


def _parts(tmp_path, world):
    return [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r), allow_pickle=True) for r in range(world)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,k,rc,first_seen,chain", [(3, 31, True, True, "dcwced"), (4, 63, False, False, ""), (1, 31, True, True, ""),
                                                                 (1, 31, True, False, "")])
def test_process_ranks_text_and_stats(oracle, tmp_path, world, k, rc, first_seen, chain):
    from katome_amd.build import contig_stats
    _spawn(world, "text", k, rc, first_seen, chain, str(tmp_path))
    parts = _parts(tmp_path, world)
    counts = [len(p["seqs"]) for p in parts]
    assert sum(counts) > 10
    for layout in ("plain", "fasta"):
        sizes = [int(p[layout + "_counts"][3]) for p in parts]
        whole = b""
        for r, p in enumerate(parts):
            nc, first, total, nb, base, total_bytes = (int(x) for x in p[layout + "_counts"])
            assert (nc, first, total) == (counts[r], sum(counts[:r]), sum(counts))
            assert (nb, base, total_bytes) == (sizes[r], sum(sizes[:r]), sum(sizes))
            text = bytes(p[layout])
            assert len(text) == nb
            seqs = p["seqs"].tolist()
            want = "".join(seqs) if layout == "plain" else "".join(">katome_%d\n%s\n" % (first + j, s) for j, s in enumerate(seqs))
            assert text.decode() == want
            assert [text[o:o + ln].decode() for o, ln in zip(p[layout + "_off"].tolist(), p[layout + "_len"].tolist())] == seqs
            whole += text
        if layout == "fasta":
            assert open(os.path.join(str(tmp_path), "all.fa"), "rb").read() == whole
            assert re.findall(rb">katome_(\d+)\n", whole) == [b"%d" % i for i in range(sum(counts))]
    # Contigs::stats on every rank: the host function over all ranks' lengths
    lengths = np.concatenate([p["kmers"] for p in parts]).astype(np.uint64) + np.uint64(k - 1)
    want = contig_stats(lengths, GLEN).astuple()
    assert all(tuple(int(x) for x in p["stats"]) == want for p in parts)
    if first_seen or world == 1:
        n, L, G, err = _input(k)
        packed = pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy()
        b, dc = _one_gpu(packed, n, L, k, rc, first_seen, chain)
        t = dc.text("fasta")
        ref_text = bytes(t.text.cpu().numpy())
        ref = [ref_text[o:o + ln].decode() for o, ln in zip(t.contig_off.cpu().tolist(), t.contig_len.cpu().tolist())]
        if first_seen:
            # all records, reordered by head id, are the one-GPU text's, none left out (a rank's merged edges are in the order of
            # its own edges, which is key order: head-id order only by packed key)
            order = np.argsort(np.concatenate([p["head"] for p in parts]), kind="stable")
            assert np.concatenate([p["seqs"] for p in parts])[order].tolist() == ref == dc.sequences()
        else:
            # one rank, by packed key: byte for byte the one-GPU text
            assert np.array_equal(parts[0]["head"], np.sort(parts[0]["head"]))
            assert bytes(parts[0]["fasta"]) == ref_text
        del t, dc
        b.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [1, 2, 4])
def test_process_ranks_stats_of_sharded_lists(tmp_path, world):
    """katome_dist_contig_stats_arrays over seeded lists with ties, giants and empty ranks: every rank gets what
    katome_contig_stats_of gives for the whole list, the statuses and their messages included (asserted inside the ranks)"""
    _spawn(world, "stats", 0, False, False, "", str(tmp_path))
    assert all(int(p["ok"][0]) == 1 for p in _parts(tmp_path, world))


# ---- the host entry on thread ranks ----------------------------------------------------------------------------------------
K, RC = 31, True
_cache = {}


def _reads(oracle):
    if "reads" not in _cache:
        n, L, G, err = _input(K)
        _cache["reads"] = (pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy(), n, L)
    return _cache["reads"]


def _unitigs(oracle, tmp_path, n_devices, stages, name="u.fa", glen=GLEN, first_seen=True, **kw):
    from katome_amd.build import GpuUnitigs
    packed, n, L = _reads(oracle)
    out = str(tmp_path / name)
    u, _ = GpuUnitigs.create_from_packed(packed, n, L, reverse_complement=RC, minimal_weight_threshold=THR, output_file=out, stages=stages,
                                         original_genome_length=glen, k=K, first_seen_order=first_seen, n_devices=n_devices,
                                         ranks_share_device=n_devices > 1, **kw)
    return u, open(out, "rb").read()


def _records(data):
    """a FASTA file -> its sequences, after checking that the headers count up from 0"""
    lines = data.decode().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    assert lines[0:-1:2] == [">katome_%d" % i for i in range(len(lines) // 2)]
    return lines[1:-1:2]


def _numbers(u):
    return (u.n_contigs, u.text_bytes, u.total_bases, u.longest, u.read_bytes, u.k, u.stats.astuple())


def _one_device(oracle, tmp_path, stages):
    if stages not in _cache:
        u, data = _unitigs(oracle, tmp_path, 1, stages, "one_%s.fa" % stages)
        assert u.n_devices == 1 and u.n_contigs > 10 and u.shrink["rank_rounds"] == 0
        _cache[stages] = (_numbers(u), data)
    return _cache[stages]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("stages", ["", "dcwced"])
def test_one_device_file_is_the_device_text(oracle, tmp_path, stages):
    numbers, data = _one_device(oracle, tmp_path, stages)
    packed, n, L = _reads(oracle)
    b, dc = _one_gpu(packed, n, L, K, RC, True, stages)
    t = dc.text("fasta")
    assert data == bytes(t.text.cpu().numpy()) and len(data) == numbers[1]
    seqs = _records(data)
    assert seqs == dc.sequences()
    assert numbers[0] == len(seqs) and numbers[2] == sum(map(len, seqs)) and numbers[3] == max(map(len, seqs)) and numbers[4] == n * L
    del t, dc
    b.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("stages", ["", "dcwced"])
@pytest.mark.parametrize("n_devices", [2, 3, 8])
def test_thread_ranks_equal_one_device(oracle, tmp_path, n_devices, stages):
    want, want_data = _one_device(oracle, tmp_path, stages)
    u, data = _unitigs(oracle, tmp_path, n_devices, stages)
    assert u.n_devices == n_devices and len(data) == u.text_bytes
    assert sorted(_records(data)) == sorted(_records(want_data))
    assert _numbers(u) == want
    assert u.shrink["longest_path"] + K - 1 == u.longest and u.shrink["rank_rounds"] > 0


@pytest.mark.timeout(300)
def test_small_chunks_write_the_same_bytes(oracle, tmp_path, monkeypatch):
    _, whole = _unitigs(oracle, tmp_path, 3, "dcwced", "whole.fa")
    monkeypatch.setenv("KATOME_DIST_TEXT_CHUNK", "1000")
    _, chunked = _unitigs(oracle, tmp_path, 3, "dcwced", "chunked.fa")
    assert chunked == whole and len(whole) > 5000


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures(golden_dir, tmp_path, i):
    """tests/shrinker.rs:33-36: 1, 92 and 233 merged edges"""
    from katome_amd.build import GpuUnitigs, InputFileType, set_global_k_sizes
    pinned = json.load(open(os.path.join(golden_dir, "pinned.json")))
    set_global_k_sizes(pinned["k"])
    out = str(tmp_path / "f.fa")
    for first_seen in (True, False):
        u, read_bytes = GpuUnitigs.create([os.path.join(golden_dir, pinned["fixtures"][i])], InputFileType.Fastq, False, output_file=out,
                                          original_genome_length=100, first_seen_order=first_seen, n_devices=3, ranks_share_device=True)
        assert u.n_contigs == pinned["shrink"]["counts"][i][1] and read_bytes == pinned["read_bytes"]["values"][i]
        assert len(_records(open(out, "rb").read())) == u.n_contigs


@pytest.mark.timeout(300)
def test_one_read_on_eight_ranks(oracle, tmp_path):
    """one read of four 31-mers, by packed key: most ranks hold no edge and write nothing"""
    from katome_amd.build import GpuUnitigs
    L = 34
    reads = oracle.synth_reads(3, 1, L, 5000, 0.0, 0)
    out = str(tmp_path / "one.fa")
    u, _ = GpuUnitigs.create_from_packed(pack_reads_ascii(reads).reshape(-1).copy(), 1, L, k=31, output_file=out, original_genome_length=34,
                                         n_devices=8, ranks_share_device=True)
    seq = reads[0].tobytes().decode()
    assert open(out, "rb").read().decode() == ">katome_0\n%s\n" % seq
    assert (u.n_contigs, u.total_bases, u.longest, u.stats.astuple()) == (1, 34, 34, (34, 1, 34, 34))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_devices", [1, 2])
def test_no_edges_at_all(oracle, tmp_path, n_devices):
    """every read is skipped: an empty file and zero stats"""
    from katome_amd.build import GpuUnitigs
    packed, n, L = _reads(oracle)
    out = str(tmp_path / "empty.fa")
    u, read_bytes = GpuUnitigs.create_from_packed(packed[:64 * ((L + 3) // 4)], 64, L, skip=np.ones(64, np.uint8), k=K, output_file=out,
                                                  original_genome_length=1000, n_devices=n_devices, ranks_share_device=n_devices > 1)
    assert open(out, "rb").read() == b"" and read_bytes == 0
    assert (u.n_contigs, u.text_bytes, u.total_bases, u.longest, u.stats.astuple()) == (0, 0, 0, 0, (0, 0, 0, 0))


@pytest.mark.timeout(300)
def test_refusals(oracle, tmp_path):
    from katome_amd.build import KatomePanic
    for kw in (dict(stages="dcwced"), dict(stages="", remove_dead_paths=True)):           # the sharded stages need the links
        for n_devices in (1, 3):
            with pytest.raises(KatomePanic) as e:
                _unitigs(oracle, tmp_path, n_devices, kw["stages"], first_seen=False, **{k: v for k, v in kw.items() if k != "stages"})
            assert e.value.name == "E_ARG" and "FIRST_SEEN" in e.value.message
    u, data = _unitigs(oracle, tmp_path, 3, "", "by_key.fa", first_seen=False)            # a packed-key build without them is fine
    assert sorted(_records(data)) == sorted(_records(_one_device(oracle, tmp_path, "")[1]))
    for n_devices in (1, 3):
        bad = tmp_path / "no_such_dir" / "u.fa"
        with pytest.raises(KatomePanic) as e:                                             # asm/mod.rs:62
            _unitigs(oracle, tmp_path, n_devices, "", os.path.join("no_such_dir", "u.fa"))
        assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
        with pytest.raises(KatomePanic) as e:                                             # a tipping point of 0: the file is still written
            _unitigs(oracle, tmp_path, n_devices, "", "tip%d.fa" % n_devices, glen=1)
        assert e.value.name == "E_ARG" and "ng50" in e.value.message
        data, one = open(str(tmp_path / ("tip%d.fa" % n_devices)), "rb").read(), _one_device(oracle, tmp_path, "")
        assert len(data) == one[0][1] and sorted(_records(data)) == sorted(_records(one[1]))


@pytest.mark.timeout(300)
def test_failure_reaches_every_rank(oracle, tmp_path, monkeypatch):
    """KATOME_DIST_TEXT_FAIL=1 on four ranks: the call returns rank 1's failure, no file is left behind; a clean run follows"""
    from katome_amd.build import KatomePanic
    monkeypatch.setenv("KATOME_DIST_TEXT_FAIL", "1")
    with pytest.raises(KatomePanic) as e:
        _unitigs(oracle, tmp_path, 4, "", "fail.fa")
    assert e.value.name == "E_UNSUPPORTED" and "rank 1" in e.value.message
    assert not os.path.exists(str(tmp_path / "fail.fa"))
    monkeypatch.delenv("KATOME_DIST_TEXT_FAIL")
    u, data = _unitigs(oracle, tmp_path, 4, "", "fail.fa")
    assert u.n_contigs > 10 and len(data) == u.text_bytes
