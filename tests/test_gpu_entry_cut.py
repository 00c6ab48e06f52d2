"""The kernels that make a list-fed level's records off the list (radix.hip ListSource, table.hip list_digit_counts_kernel) cut them
once per list entry (entry_cut.h) instead of once per record.  Through katome_dev_list_first_pass the records after the pass, their
weights and the per-tile digit counts must be byte for byte what the pass over written records gives (fused = 0), and what the
per-record cut gives (KATOME_ENTRY_CUT=0); one whole build must be equal across the switch and equal to the oracle.  The switch is
read once, so each setting runs in ONE child process of its own under a time limit -- the primitives and the build together --, started
once for the module; a child that ends any other way than with status 0 fails the tests, which start nothing more."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, tile_bases, k, span, stride, rc, rep): the two levels of k = 31 with both strands and with one, one-word tiles into k-mers, and
# the spans that divide a sort tile (4096 one-word records, 2048 two-word ones)
_FORMS = [("mid_2_2_rc", 60, 36, 5, 6, 1, 0), ("mid_2_2_one_strand", 60, 36, 5, 6, 0, 0),
          ("kmers_2_1_rc", 36, 31, 6, 1, 1, 1), ("kmers_2_1_one_strand", 36, 31, 6, 1, 0, 1),
          ("kmers_1_1_rc", 18, 13, 6, 1, 1, 1), ("kmers_1_1_one_strand", 18, 13, 6, 1, 0, 1), ("kmers_1_1_span5_rc", 17, 13, 5, 1, 1, 1),
          ("span2_2_1_rc", 32, 31, 2, 1, 1, 1), ("span4_1_1_rc", 16, 13, 4, 1, 1, 1), ("span4_2_2_rc", 63, 36, 4, 9, 1, 0), ("span2_2_2_rc", 45, 36, 2, 9, 1, 0)]


def _sort_tile(k):
    return 4096 if 2 * k <= 62 else 2048


def _last_tile_of(r, span, tile, tiles):
    """the first entry count from `tiles` sort tiles on whose records end r records into a tile, or None where span forbids it"""
    for e in range(-(-tiles * tile // span), -(-tiles * tile // span) + tile):
        if e * span % tile == r:
            return e
    return None


def _entry_counts(span, tile):
    """none; one; a last tile of one record (of two where span is even: n is then even) behind whole tiles; one tile
    exactly full where span divides it; 3 tiles + 1 record rounded up to whole entries; 65 tiles + 1 -- the tile numbering changes at
    64, and with five or six tiles and more a tile's first record lies at every offset of an entry that span and the tile size allow
    (offset of tile t = t * tile mod span: all of 0 .. 4 for span 5, the even ones for span 6 -- 4096 and 2048 are even)"""
    r = 1 if span % 2 else 2
    out = {0, 1, _last_tile_of(r, span, tile, 1), -(-(3 * tile + 1) // span), -(-(65 * tile + 1) // span)}
    if tile % span == 0:
        out.add(tile // span)
    return sorted(c for c in out if c is not None)


_SCRIPT = r"""
import sys, hashlib, random, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii, int_to_kmer, kmer_to_int, revcomp_str, int_to_words
from oracle import oracle as o
from katome_amd import _lib, device as kd
forms = eval(sys.argv[2]); counts = eval(sys.argv[3]); with_oracle = int(sys.argv[4])
L = _lib.lib()
rng = np.random.default_rng(23)
def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:24]

def first_pass(name, kind, words, cnt, form):
    (_, tile_bases, k, span, stride, rc, rep) = form
    n_tiles = 0 if kind == "none" else len(words)
    nwk = 1 if 2 * k <= 62 else 2
    sort_tile = 4096 if nwk == 1 else 2048
    d_tiles = torch.from_numpy(words.view(np.int64).reshape(-1).copy()).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32).copy()).cuda()
    n = n_tiles * span
    n_sort = (n + sort_tile - 1) // sort_tile
    got = []
    for fused in (1, 0):
        keys = torch.zeros(max(n, 1) * nwk, dtype=torch.int64, device="cuda")
        wts = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        dc = torch.zeros(max(n_sort, 1) * 256, dtype=torch.int32, device="cuda")
        st = L.katome_dev_list_first_pass(0, kd._ptr(d_tiles), kd._ptr(d_cnt), n_tiles, tile_bases, k, span, stride, rc, rep, fused,
                                          kd._ptr(keys), kd._ptr(wts), kd._ptr(dc), kd._stream())
        assert st == 0, (name, kind, n_tiles, fused, st, _lib.last_error())
        torch.cuda.synchronize()
        assert int(dc.sum().item()) == n, (name, kind, n_tiles, fused)
        got.append((keys, wts, dc))
    for a, b, what in zip(got[0], got[1], ("keys", "weights", "digit counts")):
        assert torch.equal(a, b), (name, kind, n_tiles, what)
    print("FP", name, kind, n_tiles, n, *(sha(t) for t in got[0]), int(got[0][1].to(torch.int64).sum().item()), flush=True)

def random_words(n_tiles, tile_bases, nwt):
    words = rng.integers(0, 1 << 63, size=(max(n_tiles, 1), nwt), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(max(n_tiles, 1), nwt), dtype=np.uint64)
    top_bits = 2 * tile_bases - 64 * (nwt - 1)
    if top_bits < 64:
        words[:, 0] &= np.uint64((1 << top_bits) - 1)
    return words

for form in forms:
    (name, tile_bases, k, span, stride, rc, rep) = form
    nwt = 1 if 2 * tile_bases <= 62 else 2
    for n_tiles in counts[name]:
        words = random_words(n_tiles, tile_bases, nwt)
        cnt = rng.integers(1, 1 << 16, size=max(n_tiles, 1), dtype=np.uint32)
        first_pass(name, "none" if n_tiles == 0 else "random", words, cnt, form)
    # a list of identical entries, and (even sub length) one whose every window is its own reverse complement: tiles of period 2
    # -- ATAT.., TATA.., CGCG.., GCGC.. -- at an even stride, canonical's tie in every record; 3 tiles + 1 record
    n_tiles = counts[name][-2]
    cnt = rng.integers(1, 1 << 16, size=n_tiles, dtype=np.uint32)
    first_pass(name, "identical", np.repeat(random_words(1, tile_bases, nwt), n_tiles, axis=0), cnt, form)
    if k % 2 == 0 and stride % 2 == 0:
        four = []
        for pair in ("AT", "TA", "CG", "GC"):
            tile = (pair * tile_bases)[:tile_bases]
            assert all(tile[q * stride:q * stride + k] == revcomp_str(tile[q * stride:q * stride + k]) for q in range(span))
            four.append(int_to_words(kmer_to_int(tile), nwt))
        first_pass(name, "self_complementary", np.array(four, dtype=np.uint64)[rng.integers(0, 4, size=n_tiles)], cnt, form)

# one whole build: k = 31, 150 bp, both strands -- big tiles of 30 windows, mid tiles of 6, both levels' records made by their first pass
reads = o.synth_reads(31, 3000, 150, 30000, 3e-3, 0)
print("BUILD", file=sys.stderr, flush=True)
packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
b = kd.Builder(31, True)
b.count_reads(packed, len(reads), reads.shape[1], None, first_read=0)
dg = b.finalize()
arrays = [t.cpu().numpy() for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label)]
h = hashlib.sha256()
for a in arrays:
    h.update(a.tobytes())
print("FR", dg.n_nodes, dg.n_edges, h.hexdigest(), flush=True)
if with_oracle:
    ref = o.build_ascii(reads, 31, True)
    got = sorted(zip((int_to_kmer(int(v), 31) for v in arrays[0].reshape(-1).view(np.uint64)), (int(w) for w in arrays[1])))
    assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges), (dg.n_nodes, dg.n_edges, ref.n_nodes, ref.n_edges)
    assert got == ref.multiset()
    print("ORACLE equal", flush=True)
del dg
b.close()
"""

_PER_ENTRY = "[entry_cut] once per list entry"
_PER_RECORD = "[entry_cut] once per record (KATOME_ENTRY_CUT=0)"
_MADE = "made by their first partition pass"


def _counts():
    return {f[0]: _entry_counts(f[3], _sort_tile(f[2])) for f in _FORMS}


def _child(with_oracle, **env_extra):
    env = dict(os.environ, KATOME_LC_TRACE="1", KATOME_SORTED_COUNT="2")      # (the k-mer level counted by sorting however small the input)
    env.pop("KATOME_ENTRY_CUT", None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", _SCRIPT, ROOT, repr(_FORMS), repr(_counts()), str(with_oracle)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    return out


@pytest.fixture(scope="module")
def runs():
    """(per entry, per record): the same script with the switch unset and with KATOME_ENTRY_CUT=0"""
    per_entry = _child(1)
    return per_entry, _child(0, KATOME_ENTRY_CUT="0")


def _rows(out, tag):
    return [line.split() for line in out.stdout.splitlines() if line.startswith(tag + " ")]


def test_shapes_are_the_ones_that_can_go_wrong():
    """(no GPU work: what _entry_counts hands the children)"""
    for span, tile in ((5, 2048), (5, 4096), (6, 4096)):
        c = _entry_counts(span, tile)
        assert c[0] == 0 and c[1] == 1
        r = 1 if span % 2 else 2
        assert any(e * span > tile and e * span % tile == r for e in c)  # a last tile of one record (two: span 6)
        assert any(3 * tile < e * span <= 3 * tile + span for e in c)    # 3 tiles + 1 record
        n_tiles = -(-c[-1] * span // tile)
        assert n_tiles == 66
        reachable = {t * tile % span for t in range(span)}
        assert {t * tile % span for t in range(n_tiles)} == reachable == (set(range(5)) if span == 5 else {0, 2, 4})
    for span, tile in ((2, 4096), (4, 4096), (4, 2048), (2, 2048)):
        assert tile // span in _entry_counts(span, tile)                 # one tile exactly full
    assert {(f[3], _sort_tile(f[2])) for f in _FORMS} >= {(5, 2048), (5, 4096), (6, 4096), (2, 4096), (4, 4096), (4, 2048), (2, 2048)}


def test_first_pass_off_the_list_equals_the_pass_over_written_records(runs):
    """fused against written, in the child itself (torch.equal on keys, weights and digit counts, every form, count and kind of list),
    with the entry cut and without it; and the two routes were two routes"""
    counts = _counts()
    for out, said in zip(runs, (_PER_ENTRY, _PER_RECORD)):
        rows = _rows(out, "FP")
        kinds = {(r[1], r[2]) for r in rows}
        for f in _FORMS:
            assert (f[0], "none") in kinds and (f[0], "random") in kinds and (f[0], "identical") in kinds
            assert ((f[0], "self_complementary") in kinds) == (f[2] % 2 == 0 and f[4] % 2 == 0)
        assert len(rows) == sum(len(c) for c in counts.values()) + len(_FORMS) + sum(1 for f in _FORMS if f[2] % 2 == 0 and f[4] % 2 == 0)
        primitives = out.stderr.split("BUILD")[0]
        assert primitives.count(_MADE) == primitives.count(said) == sum(1 for r in rows if int(r[3]))
    assert _PER_RECORD not in runs[0].stderr and _PER_ENTRY not in runs[1].stderr


def test_entry_cut_equals_the_cut_per_record(runs):
    """KATOME_ENTRY_CUT=0 against unset: the same keys, weights and per-tile digit counts, row for row"""
    a, b = _rows(runs[0], "FP"), _rows(runs[1], "FP")
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert x == y, (x, y)


def test_a_build_is_equal_across_the_switch_and_equal_to_the_oracle(runs):
    a, b = _rows(runs[0], "FR"), _rows(runs[1], "FR")
    assert len(a) == 1 and a == b
    assert _rows(runs[0], "ORACLE") == [["ORACLE", "equal"]]
    for out, said in zip(runs, (_PER_ENTRY, _PER_RECORD)):
        build = out.stderr.split("BUILD")[1]
        assert build.count(_MADE) == build.count(said) == 2, build[-1500:]
