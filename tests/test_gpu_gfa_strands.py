"""The unitig graph as bidirected GFA 1 (katome_dev_contigs_gfa_strands, katome_dev_gfa_strands_arrays, katome_gfa_strands_*): the
kernels on hand-made arrays against the Python model of the format (tests/gfa_strands_model.py) -- bytes and every result array --,
near-twins that must stay apart, malformed input refused, DeviceContigs.gfa(merge_strands=True) on the fixtures and on built graphs,
the builder and the two-strand result left as they were, and the host entries (file bytes on one GPU and on three ranks, a path
that cannot be made).
A segment is found through its first k-mer, so the hand-made segments have distinct first k-mers; with 4^k of them the cases of
thousands of segments run from k = 11 on."""
import json
import os

import numpy as np
import pytest

import gfa_model
import gfa_strands_model as sm
from test_gpu_gfa import device_arrays, _host, synth, N_READS, READ_LEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


# ---- the kernels on hand-made arrays -----------------------------------------------------------------------------------------
class Maker:
    """sequences whose first k-mers -- and those of their reverse complements -- are all different"""

    def __init__(self, k, rng):
        self.k, self.rng, self.used = k, rng, set()

    def random(self, n):
        return "".join(self.rng.choice(list("ACGT"), n))

    def take(self, s):
        heads = {s[:self.k], sm.revcomp(s[-self.k:])}
        if len(heads) < 2 or heads & self.used:
            return False
        self.used |= heads
        return True

    def fresh(self, n):
        """n bases that are not their own reverse complement's beginning"""
        while True:
            s = self.random(n)
            if self.take(s):
                return s

    def palindrome(self):
        """2k bases that are their own reverse complement"""
        while True:
            h = self.random(self.k)
            if h != sm.revcomp(h) and h not in self.used:
                self.used.add(h)
                return h + sm.revcomp(h)

    def near_twin(self, n, at):
        """(s, t): t = revcomp(s) but for the base that faces base `at` of s, which lies between the two end k-mers"""
        assert self.k <= at < n - self.k
        s = self.fresh(n)
        t = list(sm.revcomp(s))
        t[n - 1 - at] = "ACGT"[("ACGT".index(t[n - 1 - at]) + 1 + int(self.rng.integers(0, 3))) % 4]
        return s, "".join(t)


def _case(name, k, rng):
    """-> (n_nodes, src, dst, weight, seqs)"""
    m = Maker(k, rng)
    rc = sm.revcomp
    if name == "no_edges":
        return 3, [], [], [], []
    if name == "pair_no_links":
        s = m.fresh(k + 2)
        return 4, [0, 2], [1, 3], [5, 7], [s, rc(s)]
    if name == "pair_with_links":                  # A -> B and B' -> A', listed A, B', B, A'
        a, b = m.fresh(k + 3), m.fresh(k + 6)
        return 6, [0, 5, 1, 4], [1, 4, 2, 3], [3, 4, 5, 6], [a, rc(b), b, rc(a)]
    if name == "self_twin":                        # P -> S -> P' with S its own reverse complement: 2k bases, at k = 4 the one k-mer ACGT
        s = "ACGT" if k == 4 else m.palindrome()
        m.used |= {"ACGT"}
        p = m.fresh(k + 5)
        return 5, [0, 1, 4], [1, 4, 3], [2, 9, 3], [p, s, rc(p)]
    if name == "hairpin":                          # x ends in a vertex that is its own mirror: x -> x'
        x = m.fresh(k + 1)
        return 3, [0, 1], [1, 2], [4, 6], [x, rc(x)]
    if name == "self_loop":                        # r -> r and r' -> r': r + r + once
        r = m.fresh(k + 4)
        return 2, [1, 0], [1, 0], [8, 9], [rc(r), r]
    if name == "hub":                              # 4 edges into vertex 4 and 4 out of it, and the mirror (v <-> v + 9): 32 links, 16 lines
        src, dst = [0, 1, 2, 3, 4, 4, 4, 4], [4, 4, 4, 4, 5, 6, 7, 8]
        seqs = [m.fresh(int(x)) for x in rng.integers(k, k + 30, 8)]
        src, dst, seqs = src + [d + 9 for d in dst], dst + [s + 9 for s in src], seqs + [rc(s) for s in seqs]
        p = rng.permutation(16)
        return 18, [src[i] for i in p], [dst[i] for i in p], list(range(1, 17)), [seqs[i] for i in p]
    if name == "mirror_absent":                    # A -> B without B' -> A'; D' -> C' without C -> D
        a, b, c, d = (m.fresh(k + i) for i in range(4))
        return 14, [0, 1, 4, 5, 7, 9, 11, 12], [1, 2, 3, 6, 8, 10, 12, 13], list(range(1, 9)), [a, b, rc(a), rc(b), c, d, rc(d), rc(c)]
    if name == "every_alignment":                  # pairs of k .. k + 9 bases with a label between the members; from k = 11 on (enough
        seqs, at = [], 0                           # first k-mers) further labels put both members at every byte alignment in turn
        size = lambda n: 1 + (n + 3) // 4
        def pad_to(want):
            nonlocal at
            n = next(n for n in range(k, k + 16) if (at + size(n)) % 4 == want)
            seqs.append(m.fresh(n)); at += size(n)
        for i in range(10):
            s = m.fresh(k + i)
            if k >= 11 and at % 4 != i % 4:
                pad_to(i % 4)
            seqs.append(s); at += size(len(s))
            if k >= 11:
                pad_to((i + 2) % 4)
            else:
                seqs.append(m.fresh(k + 4 * (i % 3) + 1)); at += size(len(seqs[-1]))
            seqs.append(rc(s)); at += size(len(s))
        n = len(seqs)
        return 2 * n, list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2)), [int(x) for x in rng.integers(1, 50, n)], seqs
    if name == "near_twins":                       # one base differs: just behind the first k-mer, just before the last one, at a word's edges
        w = 16 * (k // 16 + 1)
        n = w + 2 + k + 5
        seqs = []
        for at in (k, n - k - 1, w - 1, w, w + 1):
            seqs += list(m.near_twin(n, at))
        s = m.fresh(n)
        seqs += [s, rc(s)]                         # (and a true pair of the same length)
        c = len(seqs)
        return 2 * c, list(range(0, 2 * c, 2)), list(range(1, 2 * c, 2)), [1] * c, seqs
    if name == "long_pair":                        # a 70 000-base pair, 3000 labels of exactly k bases between its members, all one chain
        s = m.fresh(70000)
        seqs = [s] + [m.fresh(k) for _ in range(3000)] + [rc(s)]
        n = len(seqs)
        return n + 1, list(range(n)), list(range(1, n + 1)), [1] * n, seqs
    if name == "long_near_twin":                   # ... differing in the last base the end k-mers do not vouch for
        s, t = m.near_twin(70000, 70000 - k - 1)
        return 4, [0, 2], [1, 3], [1, 2], [s, t]
    if name == "many_segments":                    # names and rc:i: cross 10 / 100 / 1000; weights up to 2^32 - 1; one 30 000-base member
        n = 1200
        lengths = [int(x) for x in rng.integers(k, k + 40, n // 2)]
        lengths[100] = 30000 + k - 1             # (a paired one)
        seqs = [m.fresh(x) for x in lengths]
        seqs += [rc(s) for s in seqs[:n // 4]] + [m.fresh(int(x)) for x in rng.integers(k, k + 40, n // 4)]
        p = rng.permutation(n)
        seqs = [seqs[i] for i in p]
        weight = [int(x) for x in rng.integers(1, 2 ** 32, n)]
        weight[0], weight[1100], weight[7] = 2 ** 32 - 1, 2 ** 32 - 1, 1
        return 600, [int(x) for x in rng.integers(0, 600, n)], [int(x) for x in rng.integers(0, 600, n)], weight, seqs
    raise KeyError(name)


def check_arrays(k, n_nodes, src, dst, weight, seqs):
    from katome_amd import device as kd
    args, label_bytes = device_arrays(k, src, dst, weight, seqs)
    g = kd.gfa_strands_arrays(k, n_nodes, *args, label_bytes=label_bytes)
    kmers = [len(s) - k + 1 for s in seqs]
    want, names, seg, first, twin = sm.strands_text(k, src, dst, weight, kmers, seqs)
    got = g.bytes()
    assert len(got) == g.text_bytes == len(want)
    assert got == want
    assert g.n_segments == len(names) and g.n_links == first[-1]
    assert g.segment_name.cpu().tolist() == names and g.segment_off.cpu().tolist() == seg and g.link_first.cpu().tolist() == first
    assert g.edge_twin.cpu().tolist() == twin
    assert g.n_unpaired == sum(t == sm.NO_TWIN for t in twin) and g.n_self_twins == sum(t == i for i, t in enumerate(twin))
    return g, twin


SMALL = ["no_edges", "pair_no_links", "pair_with_links", "self_twin", "hairpin", "self_loop", "hub", "mirror_absent", "every_alignment", "near_twins"]
LARGE = ["long_pair", "long_near_twin", "many_segments"]


@pytest.mark.parametrize("name,k", [(n, k) for k in (3, 4, 11, 32, 33) for n in SMALL] +
                         [(n, k) for k in (11, 32, 33) for n in LARGE])
def test_kernels_on_hand_made_arrays(name, k):
    rng = np.random.default_rng(len(name) * 131 + k)
    n_nodes, src, dst, weight, seqs = _case(name, k, rng)
    g, twin = check_arrays(k, n_nodes, src, dst, weight, seqs)
    want = {"no_edges": (0, 0, 0, 0), "pair_no_links": (1, 0, 0, 0), "pair_with_links": (2, 1, 0, 0), "self_twin": (2, 1, 0, 1), "hairpin": (1, 1, 0, 0),
            "self_loop": (1, 1, 0, 0), "hub": (8, 16, 0, 0), "mirror_absent": (4, 2, 0, 0), "near_twins": (11, 0, 10, 0), "long_pair": (3001, 3001, 3000, 0),
            "long_near_twin": (2, 0, 2, 0)}
    if name in want:
        assert (g.n_segments, g.n_links, g.n_unpaired, g.n_self_twins) == want[name]
    text = g.bytes().decode()
    if name == "self_twin":
        assert text.endswith("\nL\t0\t+\t1\t+\t%dM\n" % (k - 1)) and "\trc:i:1\trw:i:9\n" in text
    if name == "hairpin":
        assert text.endswith("\nL\t0\t+\t0\t-\t%dM\n" % (k - 1))
    if name == "self_loop":
        assert text.endswith("\nL\t0\t+\t0\t+\t%dM\n" % (k - 1)) and text.count("\nL\t") == 1
    if name == "every_alignment":
        off = np.cumsum([0] + [len(gfa_model.compress_edge(s)) for s in seqs])
        pairs = [(i, t) for i, t in enumerate(twin) if t != sm.NO_TWIN and t > i]
        assert sorted(len(seqs[i]) for i, _ in pairs) == list(range(k, k + 10)) and all(t > i + 1 for i, t in pairs)
        if k >= 11:                                # both members of the pairs start at every byte alignment
            assert {int(off[i]) % 4 for i, _ in pairs} == {0, 1, 2, 3} == {int(off[t]) % 4 for _, t in pairs}
        assert g.n_segments == len(seqs) - 10 and g.n_unpaired == len(seqs) - 20
    if name == "many_segments":
        assert g.n_unpaired == 600 and g.n_segments == 900 and "\trc:i:1" in text and max(len(ln) for ln in text.split("\n")) > 30000


def test_two_segments_with_one_first_kmer_are_refused():
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    k, rng = 11, np.random.default_rng(7)
    m = Maker(k, rng)
    seqs = [m.fresh(20), m.fresh(25), m.fresh(14)]
    seqs.append(seqs[1][:k] + m.random(9))
    args, label_bytes = device_arrays(k, [0, 1, 2, 3], [1, 2, 3, 4], [1, 1, 1, 1], seqs)
    with pytest.raises(KatomePanic) as e:
        kd.gfa_strands_arrays(k, 5, *args, label_bytes=label_bytes)
    assert e.value.name == "E_ARG" and "segments 1 and 3 start with the same k-mer" in e.value.message


def test_malformed_input_is_refused():
    """what katome_dev_gfa_arrays refuses (test_gpu_gfa.py), refused the same way"""
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    k, rng = 5, np.random.default_rng(5)
    m = Maker(k, rng)
    seqs = [m.fresh(7), m.fresh(9), m.fresh(12)]
    src, dst, weight = [0, 1, 2], [1, 2, 0], [1, 2, 3]
    good, label_bytes = device_arrays(k, src, dst, weight, seqs)
    assert kd.gfa_strands_arrays(k, 3, *good, label_bytes=label_bytes).n_links == 3

    def refused(what, n_nodes=3, label_bytes=label_bytes, **kw):
        a = dict(src=src, dst=dst, weight=weight, seqs=seqs)
        a.update(kw)
        args, _ = device_arrays(k, **a)
        with pytest.raises(KatomePanic) as e:
            kd.gfa_strands_arrays(k, n_nodes, *args, label_bytes=label_bytes)
        assert e.value.name == "E_ARG" and what in e.value.message, (what, e.value.message)

    refused("n_nodes", src=[0, 3, 2])
    refused("n_nodes", dst=[1, 2, 2 ** 40])
    refused("n_nodes", n_nodes=2)
    sizes = [len(gfa_model.compress_edge(s)) for s in seqs]
    total = sum(sizes)
    refused("offsets", off=[0, sizes[0], sizes[0] + sizes[1], total + 4])
    refused("offsets", label_bytes=total - 1)
    refused("offsets", off=[0, sizes[0] + sizes[1], sizes[0], total])
    refused("offsets", off=[0, sizes[0], sizes[0] + 1, total])
    raw = bytearray(b"".join(gfa_model.compress_edge(s) for s in seqs))
    raw[sizes[0]] = 4
    refused("pad byte", raw=bytes(raw))
    refused("shorter than k", seqs=[seqs[0], "ACGT", seqs[2]], kmers=[3, 1, 8])
    refused("edge_kmers", kmers=[3, 5, 9])
    refused("edge_kmers", kmers=[3, 2 ** 32 - 1, 8])


# ---- DeviceContigs.gfa(merge_strands=True) ------------------------------------------------------------------------------------
def check_contigs(dc, k, symmetric=False):
    """gfa(merge_strands=True) of a shrink result against the model on the arrays copied from it; symmetric: the build ran no stage,
    so wherever the model finds every segment's twin, expand() of the text is gfa() of the same result byte for byte -> the result"""
    src, dst, weight, kmers, seqs = _host(dc)
    g = dc.gfa(merge_strands=True)
    want, names, seg, first, twin = sm.strands_text(k, src, dst, weight, kmers, seqs)
    got = g.bytes()
    assert got == want
    assert (g.n_segments, g.n_links, g.text_bytes) == (len(names), first[-1], len(want))
    assert g.segment_name.cpu().tolist() == names and g.segment_off.cpu().tolist() == seg and g.link_first.cpu().tolist() == first
    assert g.edge_twin.cpu().tolist() == twin
    unpaired = sum(t == sm.NO_TWIN for t in twin)
    assert g.n_unpaired == unpaired and g.n_self_twins == sum(t == i for i, t in enumerate(twin))
    if symmetric and unpaired == 0:
        assert sm.expand(got, k) == dc.gfa().bytes()
        assert bytes(g.text.cpu().numpy()) == want          # (the two-strand call left the merged result alone)
    return g, unpaired


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "pinned.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("how", ["key31", "key40", "seen", "seen_dcwced"])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures(golden_dir, pinned, i, how):
    """reverse_complement builds of the fixtures: by key at k = 31 and k = 40 and in the reference's numbering without stages (every
    segment has its twin there: no cycle is cut on one strand alone in these fixtures), and after the stages dcwced"""
    from katome_amd import device as kd
    from katome_amd.build import ingest_files, InputFileType
    k = {"key31": 31, "key40": 40}.get(how, pinned["k"])
    r = ingest_files([os.path.join(golden_dir, pinned["fixtures"][i])], InputFileType.Fastq, k)
    b = kd.Builder(k, True, first_seen_order=how.startswith("seen"))
    b.count_reads(torch.from_numpy(r["packed"].copy()).cuda(), r["n_reads"], r["fixed_len"])
    b.finalize()
    if how == "seen_dcwced":
        for st in "dcwced":
            {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.remove_weak_edges(1), "e": lambda: b.standardize_edges(20000, 1)}[st]()
    dc = b.shrink()
    g, unpaired = check_contigs(dc, k, symmetric=how != "seen_dcwced")
    if how != "seen_dcwced":
        assert unpaired == UNPAIRED_WITHOUT_STAGES[how][i]
        assert 2 * g.n_segments - g.n_self_twins - unpaired == dc.n_edges
    del g, dc
    b.close()


# what the model counts on the oracle's shrink of the fixtures (no stages): no segment is left without its twin
UNPAIRED_WITHOUT_STAGES = {"key31": [0, 0, 0], "key40": [0, 0, 0], "seen": [0, 0, 0]}


def test_a_circular_sequence(oracle):
    """reads tiled around a 200-base circle, k = 31: each strand is one cycle, and shrink cuts the two cycles independently, so the
    model decides how many segments stay unpaired"""
    from katome_amd import device as kd
    from helpers import pack_reads_ascii
    rng = np.random.default_rng(200)
    circle = "".join(rng.choice(list("ACGT"), 200))
    reads = np.frombuffer("".join((circle * 2)[at:at + 60] for at in range(0, 200, 10)).encode(), np.uint8).reshape(20, 60)
    b = kd.Builder(31, True, first_seen_order=True)
    b.count_reads(torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda(), 20, 60)
    b.finalize()
    dc = b.shrink()
    g, unpaired = check_contigs(dc, 31)
    assert g.n_segments >= 1 and g.n_unpaired == unpaired
    del g, dc
    b.close()


@pytest.mark.parametrize("k,rc", [(31, True), (40, True), (31, False)])
def test_by_key_build_fast_shrink(oracle, k, rc):
    """synthetic reads with errors; without reverse_complement there are few or no twins, and the model still agrees"""
    from katome_amd import device as kd
    b = kd.Builder(k, rc)
    b.count_reads(torch.from_numpy(synth(oracle)).cuda(), N_READS, READ_LEN)
    b.finalize()
    dc = b.shrink("fast")
    g, unpaired = check_contigs(dc, k, symmetric=rc)
    assert g.n_segments > 10 and g.n_links > 10
    if not rc:
        assert unpaired > dc.n_edges // 2
    del g, dc
    b.close()


def test_builder_shrink_result_and_two_strand_gfa_are_left_untouched(oracle):
    from katome_amd import device as kd
    b = kd.Builder(21, True, first_seen_order=True)
    b.count_reads(torch.from_numpy(synth(oracle)).cuda(), N_READS, READ_LEN)
    b.finalize()
    b.remove_dead_paths()
    dc = b.shrink()

    def arrays():
        dg = b.graph()
        return [dg.n_nodes, dg.n_edges, dc.n_nodes, dc.n_edges, dg.edge_age is None] + [x.cpu().numpy().copy() for x in (
            dg.edge_weight, dg.edge_src, dg.edge_dst, dg.edge_key, dg.edge_label, dg.node_key, dg.edge_age, dc.edge_src, dc.edge_dst, dc.edge_weight,
            dc.edge_kmers, dc.edge_label_off, dc.edge_label, dc.node_key) if x is not None]
    before = arrays()
    two = dc.gfa()
    two_bytes, two_first = two.bytes(), two.link_first.cpu().tolist()
    g, _ = check_contigs(dc, 21)
    merged = g.bytes()
    assert g.n_segments < dc.n_edges and g.n_links > 10
    after = arrays()
    assert before[:5] == after[:5]
    for x, y in zip(before[5:], after[5:]):
        assert np.array_equal(x, y)
    assert two.bytes() == two_bytes and two.link_first.cpu().tolist() == two_first      # the earlier gfa() is still what it was
    assert dc.gfa().bytes() == two_bytes and g.bytes() == merged                       # ... and a later one leaves the merged text
    del g, two, dc
    b.close()


# ---- the host entries ----------------------------------------------------------------------------------------------------------
def _staged_model(packed, n_reads, read_len, k, rc, thr, glen, stages, first_seen):
    from katome_amd import device as kd
    b = kd.Builder(k, rc, first_seen_order=first_seen)
    b.count_reads(torch.from_numpy(packed).cuda(), n_reads, read_len)
    b.finalize()
    for st in stages:
        {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.remove_weak_edges(thr), "e": lambda: b.standardize_edges(glen, thr)}[st]()
    dc = b.shrink()
    src, dst, weight, kmers, seqs = _host(dc)
    del dc
    b.close()
    return sm.strands_text(k, src, dst, weight, kmers, seqs)


def _check_host(g, out, want, names, seg, first, twin):
    assert g.n_segments == len(names) > 10 and g.n_links == first[-1] > 10 and g.n_edges == len(twin)
    assert open(out, "rb").read() == g.text == want
    assert g.segment_name.tolist() == names and g.segment_off.tolist() == seg and g.link_first.tolist() == first
    assert g.edge_twin.view(np.int64).tolist() == twin
    assert g.n_unpaired == sum(t == sm.NO_TWIN for t in twin) and g.n_self_twins == sum(t == i for i, t in enumerate(twin))


@pytest.mark.parametrize("n_devices", [1, 3])
def test_gfa_strands_files(golden_dir, pinned, tmp_path, n_devices):
    """katome_gfa_strands_files on a fixture with the stages "dcwced" and an output path (three ranks: thread ranks on one card)"""
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, ingest_files, set_global_k_sizes
    path, out = os.path.join(golden_dir, "data3.txt"), str(tmp_path / "graph.gfa")
    k, rc, thr, glen = 12, True, 1, 20000
    set_global_k_sizes(k)
    r = ingest_files([path], InputFileType.Fastq, k)
    model = _staged_model(r["packed"].copy(), r["n_reads"], r["fixed_len"], k, rc, thr, glen, "dcwced", True)
    g = GpuGraph.gfa([path], InputFileType.Fastq, rc, thr, stages="dcwced", original_genome_length=glen, output_file=out, n_devices=n_devices,
                     ranks_share_device=n_devices > 1, merge_strands=True)
    _check_host(g, out, *model)
    assert g.read_bytes == pinned["read_bytes"]["values"][2] and g.k == k
    again = str(tmp_path / "again.gfa")
    g.save_to_file(again)                          # katome_gfa_strands_save
    assert open(again, "rb").read() == model[0]
    bad = str(tmp_path / "no_such_dir" / "graph.gfa")
    with pytest.raises(KatomePanic) as e:
        g.save_to_file(bad)
    assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
    if n_devices == 1:
        with pytest.raises(KatomePanic) as e:      # the file cannot be made: E_OPEN, and the result is handed back all the same
            GpuGraph.gfa([path], InputFileType.Fastq, rc, thr, stages="dcwced", original_genome_length=glen, output_file=bad, merge_strands=True)
        assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
        assert e.value.result is not None and e.value.result.text == model[0] and e.value.result.edge_twin.view(np.int64).tolist() == model[4]
        with pytest.raises(KatomePanic) as e:      # stage letters need the reference's numbering
            GpuGraph.gfa([path], InputFileType.Fastq, rc, thr, stages="d", first_seen_order=False, merge_strands=True)
        assert e.value.name == "E_ARG" and "FIRST_SEEN_ORDER" in e.value.message


@pytest.mark.parametrize("n_devices", [1, 3])
def test_gfa_strands_packed(oracle, tmp_path, n_devices):
    """katome_gfa_strands_packed on synthetic reads without stage letters: one GPU builds by packed key and shrinks in the fast form;
    three ranks build sharded in the reference's numbering, gather and shrink exactly"""
    from katome_amd.build import GpuGraph
    k, rc = 31, True
    packed, out = synth(oracle), str(tmp_path / "graph.gfa")
    model = _staged_model(packed, N_READS, READ_LEN, k, rc, 0, 0, "", n_devices > 1)
    g = GpuGraph.gfa_from_packed(packed, N_READS, READ_LEN, reverse_complement=rc, stages="", output_file=out, k=k, n_devices=n_devices,
                                 ranks_share_device=n_devices > 1, merge_strands=True)
    _check_host(g, out, *model)
    assert g.read_bytes == N_READS * READ_LEN
