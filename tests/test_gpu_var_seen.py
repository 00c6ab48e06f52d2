"""First-seen builds of reads of varying length with every level counted by sorting (KATOME_SEEN_VAR_SORTED=1): the batches' records
are kept aside with delta tags (katome_amd/csrc/seen_tag.h) instead of going into the HBM tables.  Array for array against the oracle's
petgraph, before and after remove_dead_paths; and no slot of a k-mer table (for one-word k-mers with tiles: of a tile table either).
Every case runs a script in a child process: the switches are read once per process."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 1500            # windows per batch of the "many batches" variants: the sequence base of all but the first is not zero


def _var_fastq(path, seed, n_reads, k, genome_len=3000, err=0.01, long_at=None):
    """reads of every length from k to ~5k off one circular genome (so they overlap, and pruning leaves the circle) with 1 % errors; read 0 has exactly k bases, read 1 is
    shorter than any tile (k + 1 bases: two windows), read 5 repeats read 3 verbatim and read 7 is the reverse complement of read 4
    (its k-mers are first seen on the other strand).  long_at: a read of 33 000 bases of its own goes in at that index"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len)
    reads = []
    for i in range(n_reads):
        n = k if i == 0 else k + 1 if i == 1 else int(rng.integers(k, 5 * k + 7))
        s0 = int(rng.integers(0, genome_len))
        r = genome[(s0 + np.arange(n)) % genome_len]
        m = rng.random(n) < err
        r[m] = rng.integers(0, 4, int(m.sum()))
        reads.append(r)
    reads[5] = reads[3].copy()
    reads[7] = (3 - reads[4])[::-1].copy()
    if long_at is not None:
        reads.insert(long_at, rng.integers(0, 4, 33000))
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, "".join("ACGT"[c] for c in r), "I" * len(r)))
    return reads


# argv: root, fastq, k, strands (1 / 2), variants ("batch:tiles" with batch = windows per batch or 0 for one batch, tiles 0 (every window on
# its own), 1 (the library's span) or a span to force -- one above 16 has a mid-tile level; or "file")
_SCRIPT = r"""
import hashlib, os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from oracle import oracle as o
from katome_amd import device as kd
fq, k, rc = sys.argv[2], int(sys.argv[3]), sys.argv[4] == "2"
seqs = [line.strip() for i, line in enumerate(open(fq)) if i % 4 == 1]
code = np.zeros(256, np.uint8)
for i, c in enumerate("ACGT"):
    code[ord(c)] = i
chunks, off = [], [0]
for s in seqs:                                   # 4 bases per byte, first base in the top bits, every read on a byte of its own
    b = code[np.frombuffer(s.encode(), np.uint8)]
    b = np.concatenate((b, np.zeros(-len(b) % 4, np.uint8))).reshape(-1, 4)
    chunks.append((b[:, 0] << 6 | b[:, 1] << 4 | b[:, 2] << 2 | b[:, 3]).astype(np.uint8))
    off.append(off[-1] + len(chunks[-1]))
packed = torch.from_numpy(np.concatenate(chunks + [np.zeros(32, np.uint8)])).cuda()
byte_off = torch.from_numpy(np.array(off, np.int64)).cuda()
lens = torch.from_numpy(np.array([len(s) for s in seqs], np.int32)).cuda()
ref, ref_pruned = o.build_files([fq], k, rc), o.build_files([fq], k, rc, remove_dead_paths=True)

def same(lab, w, s, d, n_nodes, age, want):
    ok = (n_nodes, len(w)) == (want.n_nodes, want.n_edges) and np.array_equal(lab.reshape(want.edge_label.shape), want.edge_label) and \
        np.array_equal(w.view(np.uint32), want.edge_weight) and np.array_equal(s.view(np.uint64), want.edge_src) and np.array_equal(d.view(np.uint64), want.edge_dst)
    if ok and age is not None:
        ok = np.array_equal(age.view(np.uint32).astype(np.uint64) + 1, want.edge_slot)
    return int(ok)

def arrays(dg):
    return (dg.edge_label.cpu().numpy(), dg.edge_weight.cpu().numpy(), dg.edge_src.cpu().numpy(), dg.edge_dst.cpu().numpy(), dg.n_nodes,
            dg.edge_age.cpu().numpy() if dg.edge_age is not None else None)

for variant in sys.argv[5:]:
    if variant == "file":                        # the route a user takes: katome_build_files
        from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
        set_global_k_sizes(k)
        os.environ["KATOME_VAR_BATCH_RECORDS"] = "1500"
        os.environ["KATOME_LC_TRACE"] = "1"       # (the builder is not ours to ask for its counts: the library says on stderr how it counted)
        g, _ = GpuGraph.create([fq], InputFileType.Fastq, rc, 0, first_seen_order=True)
        print("FILE", same(g.edge_label, g.edge_weight, g.edge_src, g.edge_dst, g.n_nodes, None, ref))
        continue
    batch, tiles = (int(x) for x in variant.split(":"))
    if not tiles:
        os.environ["KATOME_NO_TILES"] = "1"
    if tiles > 1:
        os.environ["KATOME_TILE_SPAN"] = str(tiles)
    b = kd.Builder(k, rc, first_seen_order=True, table_slots_hint=1 << 14)
    b.count_var_reads(packed, byte_off, lens, batch_windows=batch or None)
    os.environ.pop("KATOME_NO_TILES", None); os.environ.pop("KATOME_TILE_SPAN", None)
    dg = b.finalize()
    c = b.counts()
    a = arrays(dg)
    digest = hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a[:4])).hexdigest()[:16]
    print("CASE", variant, same(*a, ref), dg.n_edges, c["tile_slots"], c["kmer_slots"], c["span"], digest)
    dg, _ = b.remove_dead_paths()
    print("PRUNE", variant, same(*arrays(dg), ref_pruned), dg.n_edges)
    b.close()
"""


def _run(tmp_path, fq, k, rc, variants, **env):
    script = tmp_path / "var_seen.py"
    script.write_text(_SCRIPT)
    full = dict(os.environ, KATOME_SORTED_COUNT="2", KATOME_SEEN_VAR_SORTED="1")       # (=2: by sorting however few the records)
    full.update(env)
    out = subprocess.run([sys.executable, str(script), ROOT, fq, str(k), "2" if rc else "1"] + list(variants), env=full, capture_output=True,
                         text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [line.split() for line in out.stdout.splitlines()]
    cases = {r[1]: dict(same=r[2], n_edges=int(r[3]), tile_slots=int(r[4]), kmer_slots=int(r[5]), span=int(r[6]), digest=r[7]) for r in rows if r[0] == "CASE"}
    prunes = {r[1]: dict(same=r[2], n_edges=int(r[3])) for r in rows if r[0] == "PRUNE"}
    files = [r[1] for r in rows if r[0] == "FILE"]
    wanted = [v for v in variants if v != "file"]
    assert sorted(cases) == sorted(wanted) and sorted(prunes) == sorted(wanted)
    for v in wanted:
        assert cases[v]["same"] == "1" and cases[v]["n_edges"] > 0, (v, cases[v])
        assert prunes[v]["same"] == "1" and prunes[v]["n_edges"] <= cases[v]["n_edges"], (v, prunes[v], cases[v])
    assert files == ["1"] * variants.count("file")
    if "file" in variants:                       # no table at the last level there either
        said = [line for line in out.stderr.splitlines() if line.startswith("[first-seen order, reads of varying length]")]
        assert len(said) == 1 and "levels counted by sorting" in said[0], out.stderr[-2000:]
    return cases


# one batch and many, with tiles and window by window; and with tiles of 24 windows, which are broken into mid tiles of 6 first
ALL = ["0:1", "%d:1" % BATCH, "0:0", "%d:0" % BATCH, "%d:24" % BATCH]


@pytest.mark.parametrize("k,rc,n_reads", [(31, True, 1500),      # the shape of a real trimmed input
                                          (11, True, 900),       # odd k
                                          (12, True, 700),       # even k: self-complementary k-mers, weight doubled and min(P, Q)
                                          (12, False, 700),      # one strand only
                                          (40, True, 800)])      # two-word k-mers: tiles in their table, the last level by sorting
def test_array_for_array(tmp_path, k, rc, n_reads):
    fq = str(tmp_path / "var.fq")
    _var_fastq(fq, 3 * k + n_reads, n_reads, k)
    cases = _run(tmp_path, fq, k, rc, ALL + ["file"])
    assert len({c["digest"] for c in cases.values()}) == 1
    for v, c in cases.items():
        assert c["kmer_slots"] == 0, (v, c)                      # no k-mer table (without the route all of these are counted in tables)
        if k <= 31 and not v.endswith(":0"):
            assert c["span"] > 1 and c["tile_slots"] == 0, (v, c)   # no tile table either
        if k > 31 and not v.endswith(":0"):
            assert c["span"] > 1 and c["tile_slots"] > 0, (v, c)    # two-word k-mers: the tiles stay in their table


@pytest.mark.parametrize("k,n_reads", [(31, 1500), (40, 800)])
def test_switch_restores_the_table_route(tmp_path, k, n_reads):
    fq = str(tmp_path / "var.fq")
    _var_fastq(fq, 3 * k + n_reads, n_reads, k)
    variants = ["%d:1" % BATCH, "0:0"]
    on = _run(tmp_path, fq, k, True, variants)
    off = _run(tmp_path, fq, k, True, variants, KATOME_SEEN_VAR_SORTED="0")
    for v in variants:
        assert on[v]["digest"] == off[v]["digest"], v
        assert on[v]["kmer_slots"] == 0 and off[v]["kmer_slots"] > 0, (v, on[v], off[v])


@pytest.mark.parametrize("long_at", [0, 1400])
def test_a_read_that_does_not_pack(tmp_path, long_at):
    """one read of 33 000 bases (more than 32 767 windows).  As read 0 it is in the first batch -- all of the input in the one-batch
    variants, that read alone in the batched ones (a batch takes one read at least) --, so the route closes with nothing kept and
    no sequence number handed out.  As read 1400 it comes, in the batched variants, after some sixty batches were kept aside:
    their records go back into the tables with the pairs their tags spell"""
    fq = str(tmp_path / "var.fq")
    _var_fastq(fq, 3 * 31 + 1500, 1500, 31, long_at=long_at)
    cases = _run(tmp_path, fq, 31, True, ["0:1", "0:0", "%d:1" % BATCH, "%d:0" % BATCH])
    for v, c in cases.items():
        assert c["kmer_slots"] > 0, (v, c)


@pytest.mark.parametrize("level", ["mid", "last"])
def test_a_level_gives_up(tmp_path, level):
    """KATOME_SORTED_FAIL: that level reports a group too large -- the distinct tiles (or the windows kept aside) go into the tables with
    the pairs their delta tags spell (table_tagged_to_pairs)"""
    fq = str(tmp_path / "var.fq")
    _var_fastq(fq, 3 * 31 + 1500, 1500, 31)
    cases = _run(tmp_path, fq, 31, True, ALL, KATOME_SORTED_FAIL=level)
    if level == "last":
        assert all(c["kmer_slots"] > 0 for c in cases.values()), cases
