"""The bidirected GFA of the assembly (katome_dev_gfa_strand_paths_arrays, katome_dev_collapse_gfa_strands,
katome_assemble_gfa_strands_*): the path kernels and the mirror search on hand-made arrays against the Python model
(tests/gfa_strand_paths_model.py) byte for byte and array for array, every malformed input refused,
Builder.collapse_gfa(merge_strands=True) on the fixtures and after the whole pipeline -- the H / S / L part is the merged unitig
graph's, the run structure is the two-strand one, the paths expand to the two-strand paths and follow L lines --, and the host entries."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gfa_paths_model
import gfa_strand_paths_model as model
import gfa_strands_model
from helpers import pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WHOLE, NO = model.WHOLE, model.NO_TWIN
GUARD = 64
NAMES = ("n_paths", "n_jumps", "text_bytes", "n_mirrored", "n_self_mirror")


# ---- the kernels on hand-made arrays -----------------------------------------------------------------------------------------
def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt).view({np.uint32: np.int32, np.int64: np.int64}[dt]).copy()).cuda()


def run_arrays(src, dst, twin, pieces, path_cap=None, text_cap=None):
    """the raw entry on buffers filled with 0xFF, with a guard behind each -> (text buffer, counts, line_off, contig, first_piece, mirror)"""
    from katome_amd import _lib
    from katome_amd.build import KatomePanic
    L = _lib.lib()
    d_src, d_dst, d_twin, d_pieces = _dev(src, np.int64), _dev(dst, np.int64), _dev(twin, np.int64), _dev(pieces, np.uint32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    counts = (C.c_uint64 * 5)(7, 7, 7, 7, 7)
    args = (0, len(src), p(d_src), p(d_dst), p(d_twin), p(d_pieces), len(pieces))
    rc = L.katome_dev_gfa_strand_paths_arrays(*args, None, None, None, None, 0, None, 0, counts, None)
    if rc:
        assert list(counts) == [0] * 5
        raise KatomePanic(rc, _lib.last_error())
    n_paths, n_bytes = counts[0], counts[2]
    path_cap = n_paths if path_cap is None else path_cap
    text_cap = (n_bytes + 15) // 16 * 16 if text_cap is None else text_cap
    ff = lambda n: torch.full((n,), -7, dtype=torch.int64, device="cuda")
    line_off, contig, first, mirror = ff(n_paths + 1 + GUARD), ff(n_paths + GUARD), ff(n_paths + 1 + GUARD), ff(n_paths + GUARD)
    text = torch.full((max((n_bytes + 15) // 16 * 16, 16) + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    query = list(counts)
    rc = L.katome_dev_gfa_strand_paths_arrays(*args, p(line_off), p(contig), p(first), p(mirror), path_cap, p(text), text_cap, counts, None)
    if rc:
        raise KatomePanic(rc, _lib.last_error())
    assert list(counts) == query
    return text.cpu().numpy(), dict(zip(NAMES, counts)), line_off.cpu().tolist(), contig.cpu().tolist(), first.cpu().tolist(), mirror.cpu().tolist()


def run_two_strand(src, dst, pieces):
    from katome_amd import device as kd
    _, counts, _, contig, first = kd.gfa_paths_arrays(_dev(src, np.int64), _dev(dst, np.int64), _dev(pieces, np.uint32))
    return counts["n_paths"], counts["n_jumps"], contig.cpu().tolist(), first.cpu().tolist()


def check_arrays(src, dst, twin, pieces):
    want, want_off, want_contig, want_first, want_jumps = model.path_text(src, dst, twin, pieces)
    want_mirror = model.mirrors(src, dst, twin, pieces)
    text, counts, line_off, contig, first, mirror = run_arrays(src, dst, twin, pieces)
    n, n_paths = len(want), len(want_contig)
    assert counts == dict(n_paths=n_paths, n_jumps=want_jumps, text_bytes=n, n_mirrored=sum(q != model.NO_MIRROR for q in want_mirror),
                          n_self_mirror=sum(q == j for j, q in enumerate(want_mirror)))
    assert bytes(text[:n]) == want
    cap = (n + 15) // 16 * 16
    assert not text[n:cap].any()                                             # zeros up to the next multiple of 16
    assert (text[max(cap, 16):] == 0xFF).all() and len(text) == max(cap, 16) + GUARD      # ... and nothing behind it
    assert line_off[:n_paths + 1] == want_off and first[:n_paths + 1] == want_first and contig[:n_paths] == want_contig
    assert mirror[:n_paths] == want_mirror
    assert set(line_off[n_paths + 1:]) | set(first[n_paths + 1:]) | set(contig[n_paths:]) | set(mirror[n_paths:]) == {-7}
    # the run structure is the two-strand writer's
    assert run_two_strand(src, dst, pieces) == (n_paths, want_jumps, want_contig, want_first)
    return counts, want, mirror[:n_paths]


def one_vertex(n_pairs=10, n_self=2, n_alone=2):
    """every edge follows every edge: edges 0 .. n_pairs - 1, their twins n_pairs + i, then self-twins, then edges without a twin"""
    n = 2 * n_pairs + n_self + n_alone
    twin = [n_pairs + i for i in range(n_pairs)] + list(range(n_pairs)) + [2 * n_pairs + i for i in range(n_self)] + [NO] * n_alone
    return [0] * n, [0] * n, twin


def contigs_to_pieces(*contigs):
    return [i | (WHOLE if t == 0 else 0) for c in contigs for t, i in enumerate(c)]


def two_strand_chain(n):
    """a chain i -> i + 1 of n edges (vertices 0 .. n) and its other strand: edge n + i runs from vertex 2n + i + 1 to 2n + i"""
    return list(range(n)) + [2 * n + i + 1 for i in range(n)], list(range(1, n + 1)) + [2 * n + i for i in range(n)], [n + i for i in range(n)] + list(range(n))


def _case(name, rng):
    """-> (src, dst, twin, pieces)"""
    if name == "zero_pieces":
        return [0, 1], [1, 2], [1, 0], []
    if name == "one_piece":
        return [0, 1], [1, 2], [1, 0], [1 | WHOLE]
    if name == "digits":                           # ids 1 200 .. 2 399 have four digits, their reps 0 .. 1 199 one to four: a size taken from the id is wrong
        n = 1200
        src, dst, twin = two_strand_chain(n)
        pieces = []
        for c in range(n):
            if rng.random() < 0.5:                 # forward: c, c + 1, ...
                pieces += [c | WHOLE] + [c + 1 + j for j in range(int(rng.integers(0, 3))) if c + 1 + j < n]
            else:                                  # the other strand: n + c, n + c - 1, ...
                pieces += [(n + c) | WHOLE] + [n + c - 1 - j for j in range(int(rng.integers(0, 3))) if c - 1 - j >= 0]
            if rng.random() < 0.2:
                pieces.append(int(rng.integers(2 * n)))
        return src, dst, twin, pieces
    if name == "signs":                            # - on the first and on the last piece of a line, a self-twin, an edge without a twin
        src, dst, twin = one_vertex()
        return src, dst, twin, contigs_to_pieces([15, 3, 17], [12], [2, 13], [14, 4], [20, 3, 21], [22, 13, 23], [20], [23])
    if name == "twelve_jumps":                     # edges that share no vertex: every piece after the first is a jump, runs .1 to .12
        n = 13
        twin = [n + i for i in range(n)] + list(range(n))
        return [2 * i for i in range(2 * n)], [2 * i + 1 for i in range(2 * n)], twin, [5 | WHOLE, 0 | WHOLE] + [n + i if i % 2 else i for i in range(1, 13)] + [3 | WHOLE]
    if name == "jump_on_last_piece":
        return [0, 1, 5, 9, 8, 7], [1, 2, 6, 8, 7, 6], [4, 3, NO, 1, 0, NO], [0 | WHOLE, 1, 3 | WHOLE, 4, 2]
    if name == "long_then_tiny":                   # one path of 4 000 pieces round the other strand of a cycle of 1 000 edges (three tiles), then 3 000 one-piece paths
        n = 1000
        src = list(range(n)) + [n + (i + 1) % n for i in range(n)]
        dst = [(i + 1) % n for i in range(n)] + [n + i for i in range(n)]
        twin = [n + i for i in range(n)] + list(range(n))
        return src, dst, twin, [(n + 999) | WHOLE] + [n + (998 - i) % n for i in range(3999)] + [int(x) | WHOLE for x in rng.integers(0, 2 * n, 3000)]
    if name.startswith("random"):                  # random walks over a random symmetric graph of a few hundred edges
        src, dst, twin = model.symmetric_graph(rng, int(rng.integers(100, 600)))
        return src, dst, twin, model.random_walks(rng, src, dst, twin, int(rng.integers(2000, 6000)))
    raise KeyError(name)


@pytest.mark.parametrize("name", ["zero_pieces", "one_piece", "digits", "signs", "twelve_jumps", "jump_on_last_piece", "long_then_tiny", "random0", "random1", "random2"])
def test_kernels_on_hand_made_arrays(name):
    rng = np.random.default_rng(len(name) * 17 + ord(name[-1]))
    src, dst, twin, pieces = _case(name, rng)
    counts, text, _ = check_arrays(src, dst, twin, pieces)
    if name == "zero_pieces":
        assert counts == dict.fromkeys(NAMES, 0)
    if name == "one_piece":
        assert text == b"P\tkatome_0\t0-\t*\n"
    if name == "digits":
        steps = [s for _, _, line in model.parse(text) for s in line]
        assert counts["n_paths"] - counts["n_jumps"] == 1200 and counts["n_jumps"] > 100
        assert {len(str(r)) for r, o in steps if o == "-"} == {1, 2, 3, 4} and all(r < 1200 for r, _ in steps)
    if name == "signs":
        assert text.startswith(b"P\tkatome_0\t5-,3+,7-\t*\nP\tkatome_1\t2-\t*\nP\tkatome_2\t2+,3-\t*\nP\tkatome_3\t4-,4+\t*\nP\tkatome_4\t20+,3+,21+\t*\nP\tkatome_5\t22+,3-,23+\t*\n")
        assert counts["n_self_mirror"] == 2                                # [14, 4] = [twin 4, 4] and [20]
    if name == "twelve_jumps":
        assert counts["n_jumps"] == 12 and b"P\tkatome_1.10\t10+\t*\nP\tkatome_1.11\t11-\t*\nP\tkatome_1.12\t12+\t*\nP\tkatome_2\t3+" in text
    if name == "jump_on_last_piece":
        assert text.endswith(b"P\tkatome_1\t1-,0-\t*\nP\tkatome_1.1\t2+\t*\n") and counts["n_jumps"] == 1 and counts["n_mirrored"] == 2
    if name == "long_then_tiny":
        assert counts["n_paths"] == 3001 and counts["n_jumps"] == 0 and model.path_text(src, dst, twin, pieces)[1][1] > 2 * 8192
        assert text.startswith(b"P\tkatome_0\t999-,998-,") and counts["n_mirrored"] > 1000
    if name.startswith("random"):
        assert counts["n_jumps"] > 0 and counts["n_mirrored"] > 10 and b"-" in text


def mirrors_of(*contigs, graph=None):
    src, dst, twin = graph or one_vertex()
    pieces = contigs_to_pieces(*contigs)
    return check_arrays(src, dst, twin, pieces)[2]                         # (checked against the model's definition there)


def test_mirrors():
    assert mirrors_of([0, 1, 2], [12, 11, 10]) == [1, 0]                                   # a mirrored pair
    assert mirrors_of([3, 13]) == [0] and mirrors_of([20]) == [0] and mirrors_of([3, 21, 13]) == [0]      # self-mirrors
    assert mirrors_of([0, 1], [0, 1], [11, 10], [0, 1]) == [2, 2, 0, 2]                    # three identical paths and one mirror: the smallest index wins on both sides
    assert mirrors_of([7], [0, 1], [11, 10], [11, 10], [8]) == [-1, 2, 1, 1, -1]
    assert mirrors_of([0, 1, 2], [12, 14, 10]) == [-1, -1]                                 # equal length, equal end pieces, another middle
    assert mirrors_of([0, 1, 2], [12, 11]) == [-1, -1] and mirrors_of([0, 1], [10, 11]) == [-1, -1]
    assert mirrors_of([0, 22], [22, 10]) == [-1, -1] and mirrors_of([22]) == [-1]          # broken by an edge without a twin
    # a long path and its mirror among short ones: many waves add into one signature
    src, dst, twin = one_vertex(500, 0, 0)
    walk = np.random.default_rng(5).integers(0, 1000, 5000).tolist()
    back = [twin[i] for i in reversed(walk)]
    near = list(back)
    near[2500] = twin[near[2500]]
    got = mirrors_of([1], walk, [501], near, back, graph=(src, dst, twin))
    assert got == [2, 4, 0, -1, 1]


def test_two_thousand_one_piece_paths():
    """2 000 one-piece paths, all mirrors of each other in pairs"""
    src, dst, twin = one_vertex(1000, 0, 0)
    order = np.random.default_rng(3).permutation(2000).tolist()
    where = {i: j for j, i in enumerate(order)}
    counts, _, mirror = check_arrays(src, dst, twin, [i | WHOLE for i in order])
    assert counts["n_paths"] == counts["n_mirrored"] == 2000 and counts["n_self_mirror"] == 0
    assert mirror == [where[twin[i]] for i in order]


def test_binding_on_tensors():
    """device.gfa_strand_paths_arrays, the same entry on torch tensors"""
    from katome_amd import device as kd
    src, dst, twin, pieces = _case("random0", np.random.default_rng(1))
    want, want_off, want_contig, want_first, want_jumps = model.path_text(src, dst, twin, pieces)
    want_mirror = model.mirrors(src, dst, twin, pieces)
    text, counts, line_off, contig, first, mirror = kd.gfa_strand_paths_arrays(_dev(src, np.int64), _dev(dst, np.int64), _dev(twin, np.int64), _dev(pieces, np.uint32))
    assert (counts["n_paths"], counts["n_jumps"], counts["text_bytes"]) == (len(want_contig), want_jumps, len(want)) and text.numel() % 16 == 0
    assert bytes(text.cpu().numpy()[:len(want)]) == want
    assert (line_off.cpu().tolist(), contig.cpu().tolist(), first.cpu().tolist(), mirror.cpu().tolist()) == (want_off, want_contig, want_first, want_mirror)
    assert kd.unique_paths(mirror.cpu().tolist()) == [j for j, q in enumerate(want_mirror) if q == -1 or q >= j]
    assert counts["n_mirrored"] == sum(q != -1 for q in want_mirror)


def test_malformed_input_is_refused():
    """each of them KATOME_E_ARG, with a message, before anything is read through it"""
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    src, dst, twin = [0, 1, 2, 12, 11, 10], [1, 2, 0, 11, 10, 12], [5, 4, 3, 2, 1, 0]
    good = [0 | WHOLE, 1, 2, 4 | WHOLE]
    assert check_arrays(src, dst, twin, good)[0]["n_paths"] == 2

    def refused(what, pieces=good, twin=twin, **kw):
        with pytest.raises(KatomePanic) as e:
            run_arrays(src, dst, twin, pieces, **kw)
        assert e.value.name == "E_ARG" and what in e.value.message, (what, e.value.message)

    refused("neither all ones nor below n_edges", twin=[5, 4, 3, 2, 1, 6])       # a twin entry >= n_edges
    refused("neither all ones nor below n_edges", twin=[5, 4, 3, 2, 1, -2])
    refused("twin(twin(i)) != i", twin=[5, 4, 3, 2, 1, 1])                       # not an involution
    refused("twin(twin(i)) != i", twin=[5, 4, 3, 2, 1, NO])                      # edge 0 names 5, 5 names nobody
    refused("n_edges", [0 | WHOLE, 6])                                           # a piece id >= n_edges
    refused("n_edges", [0x7FFFFFFF | WHOLE])
    refused("first piece", [0, 1 | WHOLE])                                       # a first piece without WHOLE
    refused("do not fit", text_cap=16)                                           # the text is 38 bytes
    refused("do not fit", path_cap=1)
    b = kd.Builder(5, False, first_seen_order=True)
    with pytest.raises(KatomePanic) as e:                                        # collapse_gfa(merge_strands=True) before collapse()
        b.collapse_gfa(merge_strands=True)
    assert e.value.name == "E_ARG" and "collapse_gfa_strands: no collapse result" in e.value.message
    b.close()


# ---- Builder.collapse_gfa(merge_strands=True) ---------------------------------------------------------------------------------
def check_collapse_gfa_strands(b):
    """collapse("fasta"), shrink("exact") + gfa(merge_strands=True), collapse_gfa() and collapse_gfa(merge_strands=True) of one builder
    -> the DeviceGfaStrandPaths' counts and its path text"""
    fa = b.collapse("fasta")
    fasta = bytes(fa.text.cpu().numpy())
    dc = b.shrink("exact")
    merged = dc.gfa(merge_strands=True)
    hsl = merged.bytes()
    two = b.collapse_gfa()
    two_bytes = two.bytes()
    g = b.collapse_gfa(merge_strands=True)
    # the earlier results are as they were
    assert merged.bytes() == hsl and two.bytes() == two_bytes and bytes(fa.text.cpu().numpy()) == fasta
    # the H / S / L part is the merged unitig graph's GFA
    lists = lambda x: [t.cpu().tolist() for t in (x.segment_off, x.link_first, x.segment_name, x.edge_twin)]
    assert bytes(g.text.cpu().numpy()) == hsl and lists(g) == lists(merged) and g.n_edges == dc.n_edges
    assert (g.n_segments, g.n_links, g.text_bytes, g.n_unpaired, g.n_self_twins) == (merged.n_segments, merged.n_links, len(hsl), merged.n_unpaired, merged.n_self_twins)
    path_text = bytes(g.path_text.cpu().numpy())
    assert g.bytes() == hsl + path_text and g.path_bytes == len(path_text)
    # the run structure is the two-strand one, and the paths expand to the two-strand paths
    assert (g.n_paths, g.n_jumps) == (two.n_paths, two.n_jumps)
    assert g.path_contig.cpu().tolist() == two.path_contig.cpu().tolist() and g.path_first_piece.cpu().tolist() == two.path_first_piece.cpu().tolist()
    twin = g.edge_twin.cpu().tolist()
    two_paths = bytes(two.path_text.cpu().numpy())
    assert model.expand(path_text, twin) == two_paths
    lines = model.parse(path_text)
    line_off = g.path_line_off.cpu().tolist()
    assert len(lines) == g.n_paths and line_off[-1] == g.path_bytes and all(path_text[o:o + 9] == b"P\tkatome_" for o in line_off[:-1])
    # every step inside a line is an L line of the merged text, in one of its two spellings
    links = set((x, ox, y, oy) for x, ox, y, oy, _ in gfa_strands_model.parse(hsl)[1])
    for _, _, line in lines:
        for (x, ox), (y, oy) in zip(line, line[1:]):
            assert any(s in links for s in model.pair_spellings(x, ox, y, oy, twin)), (x, ox, y, oy)
    # the mirrors are the definition's
    want = model.mirrors_of_paths([ids for _, _, ids in gfa_paths_model.parse(two_paths)], twin)
    assert g.path_mirror.cpu().tolist() == want
    assert (g.n_mirrored, g.n_self_mirror) == (sum(q != -1 for q in want), sum(q == j for j, q in enumerate(want)))
    assert g.unique_paths() == [j for j, q in enumerate(want) if q == -1 or q >= j]
    counts = dict(n_paths=g.n_paths, n_jumps=g.n_jumps, n_mirrored=g.n_mirrored, n_self_mirror=g.n_self_mirror, n_unpaired=g.n_unpaired, text=path_text,
                  two_strand_text=two_paths)
    del fa, dc, merged, two, g
    return counts


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "pinned.json")) as f:
        return json.load(f)


def fixture_builder(golden_dir, pinned, i, rc):
    from katome_amd import device as kd
    from katome_amd.build import ingest_files, InputFileType
    path, k = os.path.join(golden_dir, pinned["fixtures"][i]), pinned["k"]
    r = ingest_files([path], InputFileType.Fastq, k)
    b = kd.Builder(k, rc, first_seen_order=True)
    b.count_reads(torch.from_numpy(r["packed"].copy()).cuda(), r["n_reads"], r["fixed_len"])
    b.finalize()
    return b


@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures_with_reverse_complement(golden_dir, pinned, i):
    """a reverse_complement build without pruning is strand-symmetric: every path has a mirror"""
    b = fixture_builder(golden_dir, pinned, i, True)
    c = check_collapse_gfa_strands(b)
    assert c["n_paths"] > 0 and c["n_unpaired"] == 0 and c["n_mirrored"] == c["n_paths"] and b"-" in c["text"]
    b.close()


@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures_without_reverse_complement(golden_dir, pinned, i):
    """one strand only: no '-', (next to) no mirrors, and the text is the two-strand paths' with rep = id.  With no '-' anywhere a
    mirrored path can only consist of self-twins (unitigs that are their own reverse complement), which reads do not produce but by
    chance: a tenth of the paths is far above that"""
    b = fixture_builder(golden_dir, pinned, i, False)
    c = check_collapse_gfa_strands(b)
    assert b"-" not in c["text"] and c["text"] == c["two_strand_text"] and c["n_mirrored"] <= c["n_paths"] // 10
    b.close()


N_READS, READ_LEN, GLEN = 2500, 110, 15000
_reads = {}


def synth(oracle, glen=GLEN):
    if glen not in _reads:
        ascii_reads = oracle.synth_reads(0, N_READS, READ_LEN, glen, 8e-3, 0)
        _reads[glen] = pack_reads_ascii(ascii_reads).reshape(-1).copy()
    return _reads[glen]


def test_after_the_whole_pipeline(oracle):
    """a synthetic read set after "dcwced": the pruning is not strand-symmetric, so edges without a twin and paths without a mirror are allowed"""
    from katome_amd import device as kd
    k, rc, thr = 31, True, 2
    b = kd.Builder(k, rc, first_seen_order=True)
    b.count_reads(torch.from_numpy(synth(oracle)).cuda(), N_READS, READ_LEN)
    b.finalize()
    b.remove_dead_paths()
    b.standardize_contigs()
    b.remove_weak_edges(thr)
    b.standardize_contigs()
    b.standardize_edges(GLEN, thr)
    b.remove_dead_paths()
    c = check_collapse_gfa_strands(b)
    assert c["n_paths"] > 10 and c["n_mirrored"] > 0 and b"-" in c["text"]
    b.close()


def test_tandem_repeat_with_reverse_complement():
    """the read X R R Y (|X| = |Y| = 15, |R| = 20, k = 7) built on both strands: the simple loop's seam is there on each strand --
    merging cannot heal it --, and the mirrors are found"""
    from katome_amd import device as kd
    rng = np.random.default_rng(7)
    x, r, y = ("".join(rng.choice(list("ACGT"), n)) for n in (15, 20, 15))
    read = x + r + r + y
    rows = np.frombuffer(read.encode(), np.uint8).reshape(1, -1)
    b = kd.Builder(7, True, first_seen_order=True)
    b.count_reads(torch.from_numpy(pack_reads_ascii(rows).reshape(-1).copy()).cuda(), 1, len(read))
    b.finalize()
    c = check_collapse_gfa_strands(b)
    assert c["n_jumps"] >= 1 and c["n_mirrored"] > 0
    assert any(r > 0 for _, r, _ in model.parse(c["text"]))
    b.close()


# ---- the host entries ----------------------------------------------------------------------------------------------------------
def check_host_result(a, g, two, k):
    """the merged result of assemble_gfa(merge_strands=True) against the two-strand result of the same build"""
    assert g.text[:g.text_bytes].startswith(b"H\tVN:Z:1.0\n") and g.path_text == g.text[g.text_bytes:] and len(g.path_text) == g.path_bytes and g.k == k
    segments, lks = gfa_strands_model.parse(g.text[:g.text_bytes])
    assert (g.n_segments, g.n_links) == (len(segments), len(lks)) and g.segment_name.tolist() == [s[0] for s in segments]
    assert gfa_strands_model.expand(g.text[:g.text_bytes], k) == two.text[:two.text_bytes]
    twin = g.edge_twin.tolist()
    assert len(twin) == g.n_edges == two.n_segments
    assert model.expand(g.path_text, twin) == two.path_text
    assert (g.n_paths, g.n_jumps) == (two.n_paths, two.n_jumps) and g.path_contig.tolist() == two.path_contig.tolist()
    assert g.path_first_piece.tolist() == two.path_first_piece.tolist() and g.path_line_off[-1] == g.path_bytes
    assert g.path_first_piece[-1] == a.collapse_stats["n_pieces"]
    want = model.mirrors_of_paths([ids for _, _, ids in gfa_paths_model.parse(two.path_text)], twin)
    assert [q if q < 2 ** 63 else -1 for q in g.path_mirror.tolist()] == want
    assert (g.n_mirrored, g.n_self_mirror) == (sum(q != -1 for q in want), sum(q == j for j, q in enumerate(want))) and g.n_mirrored > 0
    assert g.unique_paths() == [j for j, q in enumerate(want) if q == -1 or q >= j]


@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_gfa_strands_files(golden_dir, tmp_path, n_devices):
    """katome_assemble_gfa_strands_files on a fixture (three ranks: thread ranks on one card): the two files, and the two-strand result"""
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, set_global_k_sizes
    path = os.path.join(golden_dir, "data3.txt")
    k, rc, thr, glen = 12, True, 1, 20000
    set_global_k_sizes(k)
    fasta, gfa = str(tmp_path / "contigs.fa"), str(tmp_path / "graph.gfa")
    share = dict(n_devices=n_devices, ranks_share_device=n_devices > 1)
    a, g = GpuGraph.assemble_gfa([path], InputFileType.Fastq, rc, thr, glen, fasta_file=fasta, gfa_file=gfa, merge_strands=True, **share)
    want, two = GpuGraph.assemble_gfa([path], InputFileType.Fastq, rc, thr, glen, **share)
    assert a.n_contigs > 10 and a.contigs == want.contigs and a.stats == want.stats and a.read_bytes == want.read_bytes == g.read_bytes
    assert open(gfa, "rb").read() == g.text and len(g.text) == g.text_bytes + g.path_bytes
    assert open(fasta, "rb").read() == a.fasta
    check_host_result(a, g, two, k)
    again = str(tmp_path / "again.gfa")
    g.save_to_file(again)                          # katome_gfa_strand_paths_save
    assert open(again, "rb").read() == g.text
    if n_devices == 1:
        bad = str(tmp_path / "no_such_dir" / "graph.gfa")
        with pytest.raises(KatomePanic) as e:      # the file cannot be made: E_OPEN, and both results are handed back all the same
            GpuGraph.assemble_gfa([path], InputFileType.Fastq, rc, thr, glen, gfa_file=bad, merge_strands=True)
        assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
        assert e.value.result[0].fasta == a.fasta and e.value.result[1].text == g.text
        with pytest.raises(KatomePanic) as e:
            GpuGraph.assemble_gfa([path], InputFileType.Fastq, rc, thr, glen, fasta_file=str(tmp_path / "no_such_dir" / "contigs.fa"), gfa_file=again,
                                  merge_strands=True)
        assert e.value.name == "E_OPEN" and "contigs.fa" in e.value.message and e.value.result[1].text == g.text
        assert open(again, "rb").read() == g.text


@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_gfa_strands_packed(oracle, tmp_path, n_devices):
    """the same through katome_assemble_gfa_strands_packed on synthetic reads"""
    from katome_amd.build import GpuGraph
    k, rc, thr = 31, True, 2
    packed = synth(oracle)
    fasta, gfa = str(tmp_path / "contigs.fa"), str(tmp_path / "graph.gfa")
    args = dict(reverse_complement=rc, minimal_weight_threshold=thr, original_genome_length=GLEN, k=k, n_devices=n_devices, ranks_share_device=n_devices > 1)
    a, g = GpuGraph.assemble_gfa_from_packed(packed, N_READS, READ_LEN, fasta_file=fasta, gfa_file=gfa, merge_strands=True, **args)
    want, two = GpuGraph.assemble_gfa_from_packed(packed, N_READS, READ_LEN, **args)
    assert a.n_contigs > 10 and a.contigs == want.contigs and a.read_bytes == N_READS * READ_LEN
    assert open(gfa, "rb").read() == g.text and open(fasta, "rb").read() == a.fasta
    check_host_result(a, g, two, k)
