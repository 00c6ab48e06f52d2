"""The strand-unique assembly (katome_dev_unique_contigs_arrays, katome_dev_collapse_unique): the selection kernels, the contig
mirrors and the named text writer on hand-made arrays against the Python model (tests/unique_model.py) byte for byte and array for
array in both layouts, every malformed input refused, Builder.collapse_unique() on the fixtures, after the whole pipeline and
on a tandem repeat -- the mirrors and the kept set are the model's on the contigs' ids, the text is the filter of collapse()'s --, and
the host entries katome_assemble_unique_* (both files, both results, stats, one GPU and three ranks)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gfa_paths_model
import unique_model as model
from helpers import pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WHOLE, NO = model.WHOLE, -1
GUARD = 64
K = 5
NAMES = ("n_contigs", "n_kept", "text_bytes", "n_mirrored", "n_self_mirror")


# ---- the kernels on hand-made arrays -----------------------------------------------------------------------------------------
def compress_edge(seq):
    """compress.rs:250-271: the pad byte, then the bases 2 bits each, first base in the top bits, zero padding"""
    pad = (4 - len(seq) % 4) % 4
    codes = ["ACGT".index(c) for c in seq] + [0] * pad
    return bytes([pad] + [codes[i] << 6 | codes[i + 1] << 4 | codes[i + 2] << 2 | codes[i + 3] for i in range(0, len(codes), 4)])


def py_contigs(labels, pieces, k):
    out = []
    for p in pieces:
        if p & WHOLE:
            out.append(labels[p & ~WHOLE])
        else:
            out[-1] += labels[p][k - 1:]
    return out


def py_text(contigs, layout):
    return ("".join(contigs) if layout == "plain" else "".join(">katome_%d\n%s\n" % (i, c) for i, c in enumerate(contigs))).encode()


def random_labels(rng, lengths):
    return ["".join(rng.choice(list("ACGT"), n)) for n in lengths]


def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt).view({np.uint32: np.int32, np.int64: np.int64, np.uint8: np.uint8}[dt]).copy()).cuda()


def device_labels(labels):
    raw = [compress_edge(s) for s in labels]
    off = np.zeros(len(raw) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raw])
    return torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, np.uint8).copy()).cuda(), torch.from_numpy(off).cuda()


def run_arrays(labels, twin, pieces, layout, k=K, caps=None, raw=None):
    """the raw entry on buffers filled with a pattern, with a guard behind each -> (text buffer, counts, mirror, name, off, len).
    caps: (contig_cap, kept_cap, text_cap) as functions of the size query's answer; raw: (d_label, d_label_off, n_labels) instead of labels"""
    from katome_amd import _lib
    from katome_amd.build import KatomePanic
    L = _lib.lib()
    lab, off = raw[:2] if raw else device_labels(labels)
    n_labels = raw[2] if raw else len(labels)
    d_twin, d_pieces = _dev(twin, np.int64), _dev(pieces, np.uint32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    counts = (C.c_uint64 * 5)(7, 7, 7, 7, 7)
    args = (0, k, p(lab), p(off), n_labels, p(d_twin), p(d_pieces), len(pieces), {"plain": 0, "fasta": 1}.get(layout, layout))
    rc = L.katome_dev_unique_contigs_arrays(*args, None, 0, None, None, None, 0, None, 0, counts, None)
    if rc:
        assert list(counts) == [0] * 5
        raise KatomePanic(rc, _lib.last_error())
    n, n_kept, n_bytes = counts[0], counts[1], counts[2]
    cap = (n_bytes + 15) // 16 * 16
    contig_cap, kept_cap, text_cap = (f(v) for f, v in zip(caps or [lambda v: v] * 3, (n, n_kept, cap)))
    ff = lambda m, dt=torch.int64: torch.full((m,), -7, dtype=dt, device="cuda")
    mirror, name, k_off, k_len = ff(n + GUARD), ff(n_kept + GUARD), ff(n_kept + GUARD), ff(n_kept + GUARD, torch.int32)
    text = torch.full((max(cap, 16) + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    query = list(counts)
    rc = L.katome_dev_unique_contigs_arrays(*args, p(mirror), contig_cap, p(name), p(k_off), p(k_len), kept_cap, p(text), text_cap, counts, None)
    if rc:
        raise KatomePanic(rc, _lib.last_error())
    assert list(counts) == query
    return text.cpu().numpy(), dict(zip(NAMES, counts)), mirror.cpu().tolist(), name.cpu().tolist(), k_off.cpu().tolist(), k_len.cpu().tolist()


def check_arrays(labels, twin, contigs, k=K):
    """both layouts against the model -> (mirror, kept, the FASTA text)"""
    pieces = model.pieces_of(contigs)
    want_mirror = model.mirrors(contigs, twin)
    want_kept = model.kept(want_mirror)
    strings = py_contigs(labels, pieces, k)
    fasta = None
    for layout in ("plain", "fasta"):
        want = model.unique_text(py_text(strings, layout), want_kept, layout, [len(s) for s in strings])
        text, counts, mirror, name, off, length = run_arrays(labels, twin, pieces, layout, k)
        n, n_kept, n_bytes = len(contigs), len(want_kept), len(want)
        assert counts == dict(n_contigs=n, n_kept=n_kept, text_bytes=n_bytes, n_mirrored=sum(q != -1 for q in want_mirror),
                              n_self_mirror=sum(q == c for c, q in enumerate(want_mirror))), layout
        assert mirror[:n] == want_mirror and name[:n_kept] == want_kept
        assert bytes(text[:n_bytes]) == want, layout
        cap = (n_bytes + 15) // 16 * 16
        assert not text[n_bytes:cap].any()                                  # zeros up to the next multiple of 16
        assert (text[max(cap, 16):] == 0xFF).all() and len(text) == max(cap, 16) + GUARD      # ... and nothing behind it
        assert set(mirror[n:]) | set(name[n_kept:]) | set(off[n_kept:]) | set(length[n_kept:]) == {-7}
        raw = bytes(text[:n_bytes]).decode()
        assert [raw[o:o + ln] for o, ln in zip(off[:n_kept], length[:n_kept])] == [strings[c] for c in want_kept], layout
        if n:
            assert n_kept >= 1 and want_kept[0] == 0                       # contig 0 is its own first copy: always kept
        fasta = want
    return want_mirror, want_kept, fasta


# edges 0 .. 9 and their twins 10 .. 19, two self-twins 20 and 21, two edges without a twin 22 and 23
TWIN = [10 + i for i in range(10)] + list(range(10)) + [20, 21] + [NO, NO]
A, A_ = [0, 1, 2], [12, 11, 10]


def labels24():
    return random_labels(np.random.default_rng(24), [K + i % 7 for i in range(24)])


def test_zero_pieces_and_one_contig():
    labels = labels24()
    for layout in ("plain", "fasta"):
        text, counts, *_ = run_arrays(labels, TWIN, [], layout)
        assert counts == dict.fromkeys(NAMES, 0) and (text[:16] == 0xFF).all()      # nothing is written
    assert check_arrays(labels, TWIN, []) == ([], [], b"")
    m, kept, fasta = check_arrays(labels, TWIN, [[3, 4]])
    assert (m, kept) == ([-1], [0]) and fasta == (">katome_0\n%s%s\n" % (labels[3], labels[4][K - 1:])).encode()


HAND = {
    "pair": ([A, A_], [1, 0], [0]), "pair_other_order": ([A_, A], [1, 0], [0]),
    "copies_alternate": ([A, A_, A, A_], [1, 0, 1, 0], [0, 2]), "copies_first": ([A, A, A_], [2, 2, 0], [0, 1]),
    "copies_last": ([A_, A, A], [1, 0, 0], [0]),
    "self_mirror": ([[3, 13]], [0], [0]), "self_twin_piece": ([[20], [3, 21, 13], [20]], [0, 1, 0], [0, 1, 2]),
    "no_twin": ([[0, 22], [22, 10], [22]], [-1, -1, -1], [0, 1, 2]),
    "near_mirror": ([A, [12, 14, 10]], [-1, -1], [0, 1]),
    "same_pieces_other_order": ([A, [10, 12, 11], A_], [2, -1, 0], [0, 1]),
    "last_dropped": ([[5], A, [7], A_], [-1, 3, -1, 1], [0, 1, 2]),
    # (by the definition the FIRST contig cannot be dropped: first(0) = 0 <= mirror(0).  What can be is the contig right behind it)
    "second_dropped": ([A_, A, [7]], [1, 0, -1], [0, 2]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_cases(name):
    contigs, want_mirror, want_kept = HAND[name]
    m, kept, _ = check_arrays(labels24(), TWIN, contigs)
    assert (m, kept) == (want_mirror, want_kept)


def test_all_kept_without_twins():
    contigs = [A, A_, A, [5], [20]]
    m, kept, fasta = check_arrays(labels24(), [NO] * 24, contigs)
    assert m == [-1] * 5 and kept == [0, 1, 2, 3, 4]
    assert fasta == py_text(py_contigs(labels24(), model.pieces_of(contigs), K), "fasta")       # the full text


def test_names_and_ordinals():
    """a header's length and digits come from the NAME: ordinals and names of different widths, and the widths' steps 9 -> 10,
    99 -> 100, 999 -> 1000 between adjacent kept names.  (Contig 0 is always kept, so the smallest ordinal that can carry a
    four-digit name is 1.)"""
    n = 1102
    labels = random_labels(np.random.default_rng(1), [K + i % 9 for i in range(n)])
    twin = [1, 0] + [NO] * (n - 2)
    # contig 0 = [0], contigs 1 .. 3 its mirror (dropped), then every label once: kept names 0, 4, 5, ..., 1101 at ordinals 0, 1, 2, ...
    m, kept, fasta = check_arrays(labels, twin, [[0], [1], [1], [1]] + [[i] for i in range(2, 1100)])
    assert kept == [0] + list(range(4, 1102)) and b">katome_9\n" in fasta and b">katome_1000\n" in fasta and b">katome_3\n" not in fasta
    # contig 0 kept, 1 .. 999 dropped, 1000 kept: ordinal 1 is named 1000
    m, kept, fasta = check_arrays(labels, twin, [[0]] + [[1]] * 999 + [[5, 6]])
    assert kept == [0, 1000] and fasta == (">katome_0\n%s\n>katome_1000\n%s%s\n" % (labels[0], labels[5], labels[6][K - 1:])).encode()


TILE = 8192


@pytest.mark.parametrize("d", list(range(-12, 3)))
def test_tile_seam(d):
    """the second kept record -- named 2: contig 1 is dropped -- begins at byte TILE + d of the text, in either layout; and the
    text ends on a tile's last byte, and on the next tile's first"""
    rng = np.random.default_rng(100 + d)
    twin = [1, 0, NO]
    contigs = [[0], [1], [2]]
    for layout, head in (("fasta", 11), ("plain", 0)):                   # ">katome_0\n" and the newline behind the bases
        labels = random_labels(rng, [TILE + d - head, 33, 40])
        want = model.unique_text(py_text(labels, layout), [0, 2], layout, [len(s) for s in labels])
        text, counts, mirror, name, off, length = run_arrays(labels, twin, model.pieces_of(contigs), layout)
        assert bytes(text[:counts["text_bytes"]]) == want and name[:2] == [0, 2] and counts["n_kept"] == 2
        assert off[1] == TILE + d + (10 if layout == "fasta" else 0)
    if d in (0, 1):                                                        # the text's end: TILE + d bytes in all
        for layout, head in (("fasta", 22), ("plain", 0)):
            labels = random_labels(rng, [5000, 9, TILE + d - head - 5000])
            check = model.unique_text(py_text(labels, layout), [0, 2], layout, [len(s) for s in labels])
            text, counts, *_ = run_arrays(labels, twin, model.pieces_of(contigs), layout)
            assert counts["text_bytes"] == TILE + d == len(check) and bytes(text[:TILE + d]) == check
            assert not text[TILE + d:(TILE + d + 15) // 16 * 16].any()


def test_compaction_across_blocks():
    """3 000 one-piece contigs mirrored in pairs, alternately kept and dropped: the scatter crosses workgroups"""
    n = 1500
    labels = random_labels(np.random.default_rng(2), [K + i % 5 for i in range(2 * n)])
    twin = [n + i for i in range(n)] + list(range(n))
    m, kept, _ = check_arrays(labels, twin, [[i + n * s] for i in range(n) for s in (0, 1)])
    assert kept == list(range(0, 2 * n, 2)) and m == [c ^ 1 for c in range(2 * n)]


def long_walks():
    n = 500
    twin = [n + i for i in range(n)] + list(range(n))
    walk = np.random.default_rng(5).integers(0, 2 * n, 5000).tolist()
    back = [twin[i] for i in reversed(walk)]
    near = list(back)
    near[2500] = twin[near[2500]]
    return random_labels(np.random.default_rng(6), [K + i % 4 for i in range(2 * n)]), twin, walk, back, near


def test_long_contigs_between_short_ones():
    """a dropped contig of 5 000 pieces between kept ones: many waves add into one signature, and 5 000 pieces vanish from the list"""
    labels, twin, walk, back, _ = long_walks()
    m, kept, _ = check_arrays(labels, twin, [walk, [1], back, [3], [501]])
    assert (m, kept) == ([2, 4, 0, -1, 1], [0, 1, 3])


def test_near_mirror_at_length():
    """a kept 5 000-piece contig whose near-mirror (one piece of 5 000 differs) and whose mirror both follow it"""
    labels, twin, walk, back, near = long_walks()
    m, kept, _ = check_arrays(labels, twin, [walk, near, back])
    assert (m, kept) == ([2, -1, 0], [0, 1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random(seed):
    """piece lists over a random involution: contigs of 1 .. 15 pieces, a third of them walked again from the other end, copies"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 300))
    perm = rng.permutation(n).tolist()
    twin = [NO] * n
    for a, b in zip(perm[0::2], perm[1::2]):
        if rng.random() < 0.95:
            twin[a], twin[b] = b, a
    for a in perm[:5]:
        if twin[a] == NO:
            twin[a] = a                                                    # a few self-twins
    contigs = []
    for _ in range(400):
        r = rng.random()
        if contigs and r < 0.3:
            back = [twin[i] for i in reversed(contigs[int(rng.integers(len(contigs)))])]
            contigs.append(back if NO not in back else [int(rng.integers(n))])
        elif contigs and r < 0.4:
            contigs.append(list(contigs[int(rng.integers(len(contigs)))]))
        else:
            contigs.append(rng.integers(0, n, int(rng.integers(1, 16))).tolist())
    labels = random_labels(rng, [int(x) for x in rng.integers(K, K + 30, n)])
    m, kept, _ = check_arrays(labels, twin, contigs)
    assert 0 < len(kept) < len(contigs) and sum(q != -1 for q in m) > 50


def test_binding_on_tensors():
    """device.unique_contigs_arrays, the same entry on torch tensors"""
    from katome_amd import device as kd
    contigs = [A, A_, [3, 13], [22], A]
    labels = labels24()
    lab, off = device_labels(labels)
    strings = py_contigs(labels, model.pieces_of(contigs), K)
    for layout in ("plain", "fasta"):
        u = kd.unique_contigs_arrays(lab, off, _dev(TWIN, np.int64), _dev(model.pieces_of(contigs), np.uint32), K, layout)
        assert (u.n_contigs, u.n_kept, u.n_mirrored, u.n_self_mirror, u.layout) == (5, 4, 4, 1, layout) and u.text.numel() % 16 == 0
        assert u.contig_mirror.cpu().tolist() == [1, 0, 2, -1, 1] and u.kept_name.cpu().tolist() == [0, 2, 3, 4]
        assert u.bytes() == model.unique_text(py_text(strings, layout), [0, 2, 3, 4], layout, [len(s) for s in strings])
        assert u.contigs() == [strings[c] for c in (0, 2, 3, 4)]


def test_malformed_input_is_refused():
    """each with its status and message, before anything is read through it"""
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    labels = labels24()
    good = model.pieces_of([A, A_])
    assert run_arrays(labels, TWIN, good, "fasta")[1]["n_kept"] == 1

    def refused(what, pieces=good, twin=TWIN, layout="fasta", status="E_ARG", **kw):
        with pytest.raises(KatomePanic) as e:
            run_arrays(labels, twin, pieces, layout, **kw)
        assert e.value.name == status and what in e.value.message, (what, e.value.message)

    refused("neither all ones nor below n_edges", twin=TWIN[:23] + [24])
    refused("neither all ones nor below n_edges", twin=TWIN[:23] + [-2])
    refused("twin(twin(i)) != i", twin=TWIN[:23] + [1])
    refused("names a label that does not exist", [0 | WHOLE, 24])
    refused("names a label that does not exist", [0x7FFFFFFF | WHOLE])
    refused("first piece", [0, 1 | WHOLE])
    refused("unknown layout", layout=2)
    refused("do not fit", caps=(lambda v: v - 1, lambda v: v, lambda v: v))
    refused("do not fit", caps=(lambda v: v, lambda v: v - 1, lambda v: v))
    refused("do not fit", caps=(lambda v: v, lambda v: v, lambda v: v - 16))
    lab, off = device_labels(labels)
    bad_off = off.clone()
    bad_off[3] = bad_off[2]                                                # an empty label
    refused("malformed", [2 | WHOLE], raw=(lab, bad_off, 24))
    refused("4-byte aligned", raw=(lab[1:], off, 24))
    from katome_amd import _lib
    L = _lib.lib()
    counts = (C.c_uint64 * 5)()
    p = lambda t: C.c_void_p(t.data_ptr())
    tw, pc = _dev(TWIN, np.int64), _dev(good, np.uint32)
    # sizes the kernels do not take are refused before anything is read
    assert L.katome_dev_unique_contigs_arrays(0, K, p(lab), p(off), 24, p(tw), p(pc), 1 << 31, 1, None, 0, None, None, None, 0, None, 0, counts, None) == -10
    assert "pieces" in _lib.last_error()
    assert L.katome_dev_unique_contigs_arrays(0, K, p(lab), p(off), (1 << 32) - 1, p(tw), p(pc), 6, 1, None, 0, None, None, None, 0, None, 0, counts, None) == -10
    assert "labels" in _lib.last_error()
    assert L.katome_dev_unique_contigs_arrays(0, K, p(lab), p(off), 24, p(tw), p(pc), 6, 1, None, 0, None, None, None, 0, None, 0, None, None) == -7
    b = kd.Builder(5, False, first_seen_order=True)
    with pytest.raises(KatomePanic) as e:                                  # collapse_unique() before collapse()
        b.collapse_unique()
    assert e.value.name == "E_ARG" and "collapse_unique: no collapse result" in e.value.message
    b.close()


def test_size_query_then_exact_caps():
    """the size query writes nothing and answers what the filling call answers; exact caps are enough"""
    labels = labels24()
    contigs = [A, [5], A_, [3, 13]]
    text, counts, mirror, name, off, length = run_arrays(labels, TWIN, model.pieces_of(contigs), "fasta")
    assert (counts["n_contigs"], counts["n_kept"]) == (4, 3) and name[:3] == [0, 1, 3] and mirror[:4] == [2, -1, 0, 3]


# ---- Builder.collapse_unique() ------------------------------------------------------------------------------------------------
def check_collapse_unique(b, collapse_layout="fasta"):
    """collapse(), collapse_gfa() and collapse_gfa(merge_strands=True) of one builder, then collapse_unique() in both layouts against
    the model on the contigs' ids -> dict of counts"""
    fa = b.collapse("fasta")
    fasta = bytes(fa.text.cpu().numpy())
    strings = fa.contigs()
    two = b.collapse_gfa()
    two_bytes = two.bytes()
    merged = b.collapse_gfa(merge_strands=True)
    merged_bytes = merged.bytes()
    twin = merged.edge_twin.cpu().tolist()
    # the contigs' ids: the two-strand paths' lines, grouped by path_contig
    lines = gfa_paths_model.parse(bytes(two.path_text.cpu().numpy()))
    contigs = [[] for _ in range(len(strings))]
    runs = [0] * len(strings)
    for (c, r, ids), pc in zip(lines, two.path_contig.cpu().tolist()):
        assert c == pc
        contigs[pc] += ids
        runs[pc] += 1
    want_mirror = model.mirrors(contigs, twin)
    want_kept = model.kept(want_mirror)
    if collapse_layout != "fasta":
        plain = b.collapse(collapse_layout)                                # whatever layout the last collapse used
        assert plain.contigs() == strings
        fa, fasta = plain, bytes(plain.text.cpu().numpy())
    for layout in ("fasta", "plain"):
        u = b.collapse_unique(layout)
        # the earlier results are as they were
        assert bytes(fa.text.cpu().numpy()) == fasta and two.bytes() == two_bytes and merged.bytes() == merged_bytes
        assert u.contig_mirror.cpu().tolist() == want_mirror and u.kept_name.cpu().tolist() == want_kept
        assert (u.n_contigs, u.n_kept, u.n_mirrored, u.n_self_mirror) == (len(strings), len(want_kept), sum(q != -1 for q in want_mirror),
                                                                          sum(q == c for c, q in enumerate(want_mirror)))
        full = py_text(strings, layout)
        assert u.bytes() == model.unique_text(full, want_kept, layout, [len(s) for s in strings]) and u.text_bytes == len(u.bytes())
        assert u.contigs() == [strings[c] for c in want_kept] and u.lengths() == [len(strings[c]) for c in want_kept]
        assert u.layout == layout
    for c, q in enumerate(want_mirror):
        if q != -1:
            assert len(strings[c]) == len(strings[q])                      # lengths agree for every mirrored pair
            if c not in want_kept and runs[c] == runs[q] == 1:             # single-run: the texts are reverse complements
                assert strings[c] == model.revcomp(strings[q])
    out = dict(n_contigs=len(strings), n_kept=len(want_kept), n_mirrored=u.n_mirrored, seams=sum(r > 1 for r in runs), full=py_text(strings, "fasta"),
               unique=b.collapse_unique("fasta").bytes())
    del fa, two, merged, u
    return out


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
    """every contig is mirrored; 2 of 4, 91 of 182, 233 of 466 are kept (tests/test_unique_host.py derives them from the oracle's strings)"""
    b = fixture_builder(golden_dir, pinned, i, True)
    c = check_collapse_unique(b, "plain" if i == 1 else "fasta")
    assert (c["n_kept"], c["n_contigs"]) == [(2, 4), (91, 182), (233, 466)][i] and c["n_mirrored"] == c["n_contigs"]
    assert c["n_kept"] < c["n_contigs"]
    b.close()


@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures_without_reverse_complement(golden_dir, pinned, i):
    """one strand only: nothing is dropped, and the text equals the full text"""
    b = fixture_builder(golden_dir, pinned, i, False)
    c = check_collapse_unique(b)
    assert c["n_kept"] == c["n_contigs"] == [2, 92, 233][i] and c["unique"] == c["full"]
    b.close()


N_READS, READ_LEN, GLEN = 2500, 110, 15000


def test_after_the_whole_pipeline(oracle):
    """the synthetic read set of tests/test_gpu_gfa_strand_paths.py after "dcwced": the pruning is not strand-symmetric, so contigs
    without a mirror stay beside the mirrored ones"""
    from katome_amd import device as kd
    k, thr = 31, 2
    packed = pack_reads_ascii(oracle.synth_reads(0, N_READS, READ_LEN, GLEN, 8e-3, 0)).reshape(-1).copy()
    b = kd.Builder(k, True, first_seen_order=True)
    b.count_reads(torch.from_numpy(packed).cuda(), N_READS, READ_LEN)
    b.finalize()
    b.remove_dead_paths()
    b.standardize_contigs()
    b.remove_weak_edges(thr)
    b.standardize_contigs()
    b.standardize_edges(GLEN, thr)
    b.remove_dead_paths()
    c = check_collapse_unique(b)
    assert c["n_contigs"] > 10 and 0 < c["n_mirrored"] and c["n_kept"] < c["n_contigs"]
    b.close()


def test_tandem_repeat_with_reverse_complement():
    """the read X R R Y (|X| = |Y| = 15, |R| = 20, k = 7) built on both strands: contigs with seams are still one sequence of ids"""
    from katome_amd import device as kd
    rng = np.random.default_rng(7)
    x, r, y = ("".join(rng.choice(list("ACGT"), n)) for n in (15, 20, 15))
    read = x + r + r + y
    rows = np.frombuffer(read.encode(), np.uint8).reshape(1, -1)
    b = kd.Builder(7, True, first_seen_order=True)
    b.count_reads(torch.from_numpy(pack_reads_ascii(rows).reshape(-1).copy()).cuda(), 1, len(read))
    b.finalize()
    c = check_collapse_unique(b)
    assert c["seams"] >= 1 and c["n_mirrored"] > 0 and c["n_kept"] < c["n_contigs"]
    b.close()


# ---- the host entries ----------------------------------------------------------------------------------------------------------
def check_host_result(a, u, want, glen):
    """(Assembly, UniqueAssembly) of assemble_unique against the Assembly of assemble() on the same input"""
    from katome_amd.build import contig_stats
    assert a.contigs == want.contigs and a.fasta == want.fasta and a.stats == want.stats and a.n_contigs == want.n_contigs      # asm_out is katome_assemble_*'s
    assert a.read_bytes == want.read_bytes == u.read_bytes and u.k == a.k and u.n_contigs == a.n_contigs
    mirror = [q if q < 2 ** 63 else -1 for q in u.contig_mirror.tolist()]
    assert len(mirror) == a.n_contigs and u.names == model.kept(mirror) and u.n_kept == len(u.names) < a.n_contigs
    assert (u.n_mirrored, u.n_self_mirror) == (sum(q != -1 for q in mirror), sum(q == c for c, q in enumerate(mirror))) and u.n_mirrored > 0
    assert all(mirror[q] != -1 and len(a.contigs[c]) == len(a.contigs[q]) for c, q in enumerate(mirror) if q != -1)
    assert u.fasta == model.unique_text(a.fasta, u.names, "fasta") and u.contigs == [a.contigs[c] for c in u.names]
    assert u.stats == contig_stats([len(s) for s in u.contigs], glen)
    return mirror


@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_unique_files(golden_dir, tmp_path, n_devices):
    """katome_assemble_unique_files on a fixture (three ranks: thread ranks on one card): the two files and both results"""
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, set_global_k_sizes
    path = os.path.join(golden_dir, "data3.txt")
    k, rc, thr, glen = 12, True, 1, 20000
    set_global_k_sizes(k)
    fasta, uniq = str(tmp_path / "contigs.fa"), str(tmp_path / "unique.fa")
    share = dict(n_devices=n_devices, ranks_share_device=n_devices > 1)
    a, u = GpuGraph.assemble_unique([path], InputFileType.Fastq, rc, thr, glen, fasta_file=fasta, unique_file=uniq, **share)
    want = GpuGraph.assemble([path], InputFileType.Fastq, rc, thr, glen, **share)
    assert a.n_contigs > 10
    check_host_result(a, u, want, glen)
    assert open(fasta, "rb").read() == a.fasta and open(uniq, "rb").read() == u.fasta
    again = str(tmp_path / "again.fa")
    u.save_to_file(again)                          # katome_unique_assembly_save
    assert open(again, "rb").read() == u.fasta
    if n_devices == 1:
        bad = str(tmp_path / "no_such_dir" / "unique.fa")
        with pytest.raises(KatomePanic) as e:      # the file cannot be made: E_OPEN, and both results are handed back all the same
            GpuGraph.assemble_unique([path], InputFileType.Fastq, rc, thr, glen, unique_file=bad)
        assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
        assert e.value.result[0].fasta == a.fasta and e.value.result[1].fasta == u.fasta
        with pytest.raises(KatomePanic) as e:      # the FASTA path fails first: it is the one reported, and the other file is still written
            GpuGraph.assemble_unique([path], InputFileType.Fastq, rc, thr, glen, fasta_file=str(tmp_path / "no_such_dir" / "contigs.fa"), unique_file=again)
        assert e.value.name == "E_OPEN" and "contigs.fa" in e.value.message and e.value.result[1].fasta == u.fasta
        assert open(again, "rb").read() == u.fasta
        from katome_amd import _lib                # nothing asked for: refused before anything is built
        from katome_amd.build import make_settings
        s = make_settings(k, first_seen_order=True)
        assert _lib.lib().katome_assemble_unique_files(C.byref(s), (C.c_char_p * 1)(os.fsencode(path)), 1, glen, None, None, None, None) == -7


@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_unique_packed(oracle, tmp_path, n_devices):
    """the same through katome_assemble_unique_packed on the synthetic reads; the mirrors are Builder.collapse_unique()'s after the
    same stages (which test_after_the_whole_pipeline holds against the model)"""
    from katome_amd import device as kd
    from katome_amd.build import GpuGraph
    k, rc, thr = 31, True, 2
    packed = pack_reads_ascii(oracle.synth_reads(0, N_READS, READ_LEN, GLEN, 8e-3, 0)).reshape(-1).copy()
    fasta, uniq = str(tmp_path / "contigs.fa"), str(tmp_path / "unique.fa")
    args = dict(reverse_complement=rc, minimal_weight_threshold=thr, original_genome_length=GLEN, k=k, n_devices=n_devices, ranks_share_device=n_devices > 1)
    a, u = GpuGraph.assemble_unique_from_packed(packed, N_READS, READ_LEN, fasta_file=fasta, unique_file=uniq, **args)
    want = GpuGraph.assemble_from_packed(packed, N_READS, READ_LEN, **args)
    assert a.n_contigs > 10 and a.read_bytes == N_READS * READ_LEN
    mirror = check_host_result(a, u, want, GLEN)
    assert open(fasta, "rb").read() == a.fasta and open(uniq, "rb").read() == u.fasta
    b = kd.Builder(k, rc, first_seen_order=True)
    b.count_reads(torch.from_numpy(packed).cuda(), N_READS, READ_LEN)
    b.finalize()
    b.remove_dead_paths()
    b.standardize_contigs()
    b.remove_weak_edges(thr)
    b.standardize_contigs()
    b.standardize_edges(GLEN, thr)
    b.remove_dead_paths()
    b.collapse("fasta")
    du = b.collapse_unique()
    assert du.contig_mirror.cpu().tolist() == mirror and du.kept_name.cpu().tolist() == u.names and du.bytes() == u.fasta
    del du
    b.close()
