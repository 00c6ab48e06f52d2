"""Tile tails and group tails of the kernels whose guarded loads were taken out of their unrolled loops: a whole tile loads without a
test, a pass's last tile (or a group's last turn) clamps or tests its index, and a lane past the end must neither count, rank nor
write what it read.

  radix_hist_kernel, radix_scatter_kernel (ArraySource)   katome_dev_sort at one and two key words, keys alone and with values, and
                                                          katome_dev_partition at one to three (katome_dev_sort takes one or two),
                                                          n around the sort tile T of the width: 4096, 2048, 1280 records
  lds_count_full_kernel, plain and counted                katome_dev_count_in_key, packed = 0 and 1, groups of one lane, one turn
                                                          (LC_THREADS * KATOME_LC_LU = 4096 records) and one turn +- 1
  group_merge_kernel                                      both-strand builds whose S2 groups hold 0 .. more than 12 * 1024 keys, on
                                                          three routes, one of them against the oracle
  src_write_kernel, both forms                            katome_dev_source_ids, and one-strand builds of exactly E edges (labels
                                                          written with the source ids), E around its block of 2048 edges

Device buffers are exactly as long as their n.  The switches are read once, so every route runs in a child process of its own,
started once for the module; a child that ends any other way than with status 0 fails its tests."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT_TILE = {1: 4096, 2: 2048, 3: 1280}           # SortTile<NW>::KEYS (radix.hip)


def _lengths(nw):
    t = SORT_TILE[nw]
    return [1, 255, 256, 257, t - 1, t, t + 1, 2 * t + 3]


def _keys(rng, n, nw, few):
    """[n, nw] uint64, most significant word first; few: so few distinct keys that equal ones meet in every tile"""
    if few:
        a = np.zeros((n, nw), np.uint64)
        a[:, nw - 1] = rng.integers(0, 7, size=n, dtype=np.uint64) << np.uint64(40)
        a[:, 0] |= rng.integers(0, 3, size=n, dtype=np.uint64)
        return a
    a = rng.integers(0, 2 ** 63, size=(n, nw), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, nw), dtype=np.uint64)
    a[:, 0] &= np.uint64((1 << 60) - 1)             # (never the all-ones record, which a partition drops)
    return a


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def _from_dev(t, nw):
    return t.cpu().numpy().view(np.uint64).reshape(-1, nw)


# ---- katome_dev_sort ----------------------------------------------------------------------------------
@pytest.mark.parametrize("few", [False, True])
@pytest.mark.parametrize("values", [False, True])
@pytest.mark.parametrize("nw", [1, 2])
def test_sort_around_the_tile(nw, values, few):
    """every pass's histogram and scatter at a whole tile, a tile and a bit, and a bit: against numpy's stable sort, byte for byte"""
    from katome_amd import device as kd
    for n in _lengths(nw):
        rng = np.random.default_rng(1000 * nw + n)
        a = _keys(rng, n, nw, few)
        v = np.arange(n, dtype=np.uint32)[::-1].copy()
        d = _to_dev(a)
        dv = torch.from_numpy(v.view(np.int32).copy()).cuda() if values else None
        assert d.numel() == n * nw
        kd.sort_keys(d, 64 * nw, nw, dv)
        torch.cuda.synchronize()
        order = np.lexsort(tuple(a[:, j] for j in range(nw - 1, -1, -1)))          # (stable)
        assert _from_dev(d, nw).tobytes() == a[order].tobytes(), (nw, n)
        if values:
            assert dv.cpu().numpy().view(np.uint32).tobytes() == v[order].tobytes(), (nw, n)


# ---- katome_dev_partition ------------------------------------------------------------------------------
@pytest.mark.parametrize("values", [False, True])
@pytest.mark.parametrize("nw", [1, 2, 3])
def test_partition_around_the_tile(nw, values):
    """one stable pass by owner, against katome_key_owner on the host; key_words 2 without values is the issue's case, the other
    widths run the same template"""
    from katome_amd import device as kd
    n_parts = 5
    b = kd.Builder(31, True)
    try:
        for n in _lengths(nw):
            rng = np.random.default_rng(77 * nw + n)
            a = _keys(rng, n, nw, False)
            vals = torch.arange(n, dtype=torch.int32, device="cuda") if values else None
            res = b.partition(_to_dev(a), n_parts, key_words=nw, values=vals)
            torch.cuda.synchronize()
            owners = np.array([kd.key_owner([int(x) for x in row], n_parts) for row in a])
            assert res[1] == [int((owners == p).sum()) for p in range(n_parts)], (nw, n)
            order = np.argsort(owners, kind="stable")
            assert _from_dev(res[0], nw).tobytes() == a[order].tobytes(), (nw, n)
            if values:
                assert res[2].cpu().numpy().tolist() == order.tolist(), (nw, n)
    finally:
        b.close()


# ---- src_write_kernel ----------------------------------------------------------------------------------
EDGES = [1, 2047, 2048, 2049, 4097]


def _sorted_edges(rng, n, k):
    """n distinct k-mers, ascending, with runs that share their source (key >> 2): every second one differs from the one before in its
    last base only where that keeps them distinct"""
    full = (1 << (2 * k)) - 1
    ints = set()
    while len(ints) < n:
        v = (int(rng.integers(0, 2 ** 62)) * int(rng.integers(1, 2 ** 62))) & full
        ints.add(v)
        if len(ints) < n and rng.integers(0, 2):
            ints.add(v ^ 1)
    return sorted(ints)


def _edge_words(ints, nw):
    return np.array([[(v >> 64) & (2 ** 64 - 1), v & (2 ** 64 - 1)][2 - nw:] for v in ints], dtype=np.uint64).reshape(-1, nw)


@pytest.mark.parametrize("k", [31, 40])
def test_source_ids_around_the_block(k):
    from katome_amd import device as kd
    from helpers import words_to_int
    nw = kd.record_words(k)
    for n in EDGES:
        ints = _sorted_edges(np.random.default_rng(k * 10000 + n), n, k)
        nodes, src = kd.source_ids(_to_dev(_edge_words(ints, nw)), k)
        torch.cuda.synchronize()
        want_nodes = sorted({v >> 2 for v in ints})
        assert [words_to_int(r) for r in _from_dev(nodes, nw)] == want_nodes, (k, n)
        pos = {v: i for i, v in enumerate(want_nodes)}
        assert src.cpu().tolist() == [pos[v >> 2] for v in ints], (k, n)


_COMMON = r"""
import ctypes as C, sys, hashlib, random, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii, kmer_to_int, int_to_kmer, words_to_int
from oracle import oracle as o
from katome_amd import _lib, device as kd

def as_rows(reads):
    return np.array([np.frombuffer(s.encode(), dtype=np.uint8) for s in reads])
"""

# one-strand builds of exactly E edges: reads x windows = E, every window a k-mer of its own.  finalize writes the labels with the
# source ids (src_write_kernel<NW, true>), which no entry point of its own runs
_LABELS_SCRIPT = _COMMON + r"""
SHAPES = {1: (1, 1), 2047: (89, 23), 2048: (64, 32), 2049: (683, 3), 4097: (241, 17)}
for k in (31, 40):
    nw = kd.record_words(k)
    o.set_k(k)
    for E, (n_reads, windows) in SHAPES.items():
        rng = random.Random(k * 10000 + E)
        while True:
            reads = ["".join(rng.choice("ACGT") for _ in range(windows + k - 1)) for _ in range(n_reads)]
            kmers = [r[i:i + k] for r in reads for i in range(windows)]
            if len(set(kmers)) == E:
                break
        print("CASE", k, E, file=sys.stderr, flush=True)
        rows = as_rows(reads)
        packed = torch.from_numpy(pack_reads_ascii(rows).reshape(-1).copy()).cuda()
        b = kd.Builder(k, False)
        b.count_reads(packed, n_reads, rows.shape[1], None, first_read=0)
        dg = b.finalize()
        assert dg.n_edges == E, (k, E, dg.n_edges)
        ints = sorted(kmer_to_int(s) for s in kmers)
        ek = [words_to_int(r) for r in dg.edge_key.cpu().numpy().view(np.uint64).reshape(-1, nw)]
        assert ek == ints, (k, E)
        srcs = sorted({v >> 2 for v in ints})
        nk = [words_to_int(r) for r in dg.node_key.cpu().numpy().view(np.uint64).reshape(-1, nw)]
        assert nk[:len(srcs)] == srcs, (k, E)
        pos = {v: i for i, v in enumerate(srcs)}
        assert dg.edge_src.cpu().tolist() == [pos[v >> 2] for v in ints], (k, E)
        lab = dg.edge_label.cpu().numpy().reshape(E, -1)
        assert lab.tobytes() == kd.labels(dg.edge_key.reshape(-1), k).cpu().numpy().tobytes(), (k, E)
        for e in sorted({0, E // 2, E - 1}):
            assert bytes(lab[e]) == o.compress_edge(int_to_kmer(ints[e], k).encode()), (k, E, e)
        print("LB", k, E, flush=True)
        del dg
        b.close()
"""


def test_labels_with_the_source_ids_around_the_block():
    env = dict(os.environ, KATOME_LC_TRACE="1")
    env.pop("KATOME_LABELS_IN_IDS", None)
    out = subprocess.run([sys.executable, "-c", _LABELS_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("LB ")] == [[str(k), str(e)] for k in (31, 40) for e in EDGES]
    assert out.stderr.count("[node ids] labels written with the source ids") == 2 * len(EDGES), out.stderr[-3000:]


# ---- lds_count_full_kernel -----------------------------------------------------------------------------
# A list entry met r times gives each of its `span` sub-windows a hash group of r records (more, where two sub-windows share a
# group): one lane, one turn of 1024 threads x 4 records and one +- 1, two turns + 1, and a turn of one record per thread +- 1.
# The level's last non-empty group ends at the array's last record.
GROUP_SIZES = [1, 1023, 1024, 1025, 4095, 4096, 4097, 8193]

_COUNT_SCRIPT = _COMMON + r"""
SIZES = eval(sys.argv[2])
L = _lib.lib()
rng = np.random.default_rng(5)
tile_bases, sub, span, stride = 60, 36, 5, 6          # the headline build's mid level
M32 = (1 << 32) - 1

def rc_int(x, k):
    y = 0
    for _ in range(k):
        y = (y << 2) | (3 - (x & 3)); x >>= 2
    return y

for rc in (0, 1):
    tiles, counts = [], []
    for r in SIZES:
        t = int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * tile_bases)) - 1)
        tiles += [t] * r
        counts += [int(c) for c in rng.integers(1, 1 << 12, size=r)]
    perm = rng.permutation(len(tiles))
    tiles = [tiles[i] for i in perm]; counts = [counts[i] for i in perm]
    n_tiles = len(tiles); n = n_tiles * span
    mask = (1 << (2 * sub)) - 1
    want, sizes = {}, {}
    for t, c in zip(tiles, counts):
        for q in range(span):
            w = (t >> (2 * (tile_bases - sub - q * stride))) & mask
            if rc:
                w = min(w, rc_int(w, sub))
            want[w] = (want.get(w, 0) + c) & M32
            sizes[w] = sizes.get(w, 0) + 1
    assert sorted(set(sizes.values())) == sorted(SIZES), sorted(set(sizes.values()))
    words = np.array([[t >> 64, t & ((1 << 64) - 1)] for t in tiles], dtype=np.uint64)
    d_tiles = torch.from_numpy(words.view(np.int64).reshape(-1).copy()).cuda()
    d_cnt = torch.from_numpy(np.array(counts, dtype=np.uint32).view(np.int32).copy()).cuda()
    got = []
    for packed in (1, 0):
        print("LEVEL", rc, packed, file=sys.stderr, flush=True)
        pk = [torch.zeros(n * 2, dtype=torch.int64, device="cuda") for _ in range(2)]
        pw = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        ok = torch.zeros(n * 2, dtype=torch.int64, device="cuda"); ow = torch.zeros(n, dtype=torch.int32, device="cuda")
        n_out = C.c_uint64(0); took = C.c_int(-1)
        st = L.katome_dev_count_in_key(0, kd._ptr(d_tiles), kd._ptr(d_cnt), n_tiles, tile_bases, sub, span, stride, rc, packed, kd._ptr(pk[0]), kd._ptr(pw[0]),
                                       kd._ptr(pk[1]), kd._ptr(pw[1]), kd._ptr(ok), kd._ptr(ow), C.byref(n_out), C.byref(took), kd._stream())
        assert st == 0, (rc, packed, st, _lib.last_error())
        torch.cuda.synchronize()
        assert took.value == packed, (rc, packed, took.value)
        m = int(n_out.value)
        keys = ok.cpu().numpy().view(np.uint64).reshape(-1, 2)[:m]; w = ow.cpu().numpy().view(np.uint32)[:m]
        got.append((pk, pw, sorted(((int(a) << 64) | int(b), int(c)) for (a, b), c in zip(keys, w))))
    for p in range(2):
        assert torch.equal(got[0][0][p], got[1][0][p]), (rc, "keys after pass", p + 1)
        assert torch.equal(got[0][1][p], got[1][1][p]), (rc, "weights after pass", p + 1)
    assert got[0][2] == got[1][2], (rc, "packed against plain")
    assert got[0][2] == sorted(want.items()), (rc, "against the dictionary", len(got[0][2]), len(want))
    print("CT", rc, n, len(want), flush=True)
"""
_FULL = "[lds count] whole keys in the slots (7 per thread): code 0"


def test_count_groups_around_a_turn():
    """both forms of lds_count_full_kernel (KATOME_LC_FULL=1 offers them lists this small) equal a dictionary sum and each other, and
    so do the records after both partition passes"""
    env = dict(os.environ, KATOME_LC_TRACE="1", KATOME_SORTED_COUNT="2", KATOME_LC_FULL="1")
    for name in ("KATOME_COUNT_IN_KEY", "KATOME_LC_FULL_PER", "KATOME_ENTRY_CUT", "KATOME_FUSED_RECORDS", "KATOME_FUSED_HIST"):
        env.pop(name, None)
    out = subprocess.run([sys.executable, "-c", _COUNT_SCRIPT, ROOT, repr(GROUP_SIZES)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    n = 5 * sum(GROUP_SIZES)
    assert [line.split() for line in out.stdout.splitlines() if line.startswith("CT ")] == [["CT", str(rc), str(n), "40"] for rc in (0, 1)]
    levels = out.stderr.split("LEVEL ")[1:]
    assert len(levels) == 4 and all(_FULL in lv for lv in levels), out.stderr[-3000:]


# ---- group_merge_kernel --------------------------------------------------------------------------------
# test_gpu_lds_order's crowded group: a read A x 8 + 15 bases + T x 8 (+ 29 of C and G) puts its 31-mer's representative into S1's
# group 0 and the reverse complement into S2's group 0, so N such reads make an S2 group of N keys: none past the merge's first
# load chunk (1), one row of its 1024 threads and one +- 1, and more than twelve rows.  "cg_only": reads of C and G alone -- no
# k-mer on either strand begins with A x 8 or T x 8, so the first and the last of the 65536 groups are empty (and most in between)
_MERGE_SCRIPT = _COMMON + r"""
COMP = str.maketrans("ACGT", "TGCA")

def crowded(seed, n):
    rng = random.Random(seed)
    seen, reads = set(), []
    while len(reads) < n:
        mid = "".join(rng.choice("ACGT") for _ in range(15))
        if mid[0] == "A" or mid[-1] == "T" or "A" * 8 in mid or "T" * 8 in mid:
            continue
        r = "A" * 8 + mid + "T" * 8
        rc = r.translate(COMP)[::-1]
        if r in seen or rc in seen:
            continue
        seen.add(r)
        reads.append(r + "".join(rng.choice("CG") for _ in range(29)))
    return reads

def digest(name, reads, k):
    print("CASE", name, file=sys.stderr, flush=True)
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, True)
    b.count_reads(packed, len(reads), reads.shape[1], None, first_read=0)
    dg = b.finalize()
    h = hashlib.sha256()
    for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
        h.update(t.cpu().numpy().tobytes())
    top = (dg.edge_key.cpu().numpy().view(np.uint64) >> np.uint64(2 * k - 16)) if k <= 32 else None
    print("MG", name, dg.n_nodes, dg.n_edges, int(top.min()), int(top.max()), h.hexdigest(), flush=True)
    b.close()

for n in (1, 1023, 1024, 1025, 12 * 1024 + 5):
    digest("crowded_%d" % n, as_rows(crowded(n, n)), 31)
rng = random.Random(3)
digest("cg_only", as_rows(["".join(rng.choice("CG") for _ in range(90)) for _ in range(400)]), 31)
for k in (11, 13):
    digest("k%d" % k, o.synth_reads(k, 4000, 150, 30000, 3e-3, 0), k)

if sys.argv[2] == "oracle":
    from katome_amd.build import GpuGraph
    k = 31
    reads = as_rows(crowded(1025, 1025))
    g, rb = GpuGraph.create_from_packed(pack_reads_ascii(reads).reshape(-1), len(reads), reads.shape[1], reverse_complement=True, k=k)
    ref = o.build_ascii(reads, k, True)
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges), (g.n_nodes, g.n_edges, ref.n_nodes, ref.n_edges)
    ek = g.key_ints("edge")
    assert ek == sorted(kmer_to_int(s) for s in ref.kmer_strings())
    assert g.multiset() == ref.multiset()
    nk = g.key_ints("node")
    assert len(set(nk)) == len(nk) == g.n_nodes
    mask = (1 << (2 * (k - 1))) - 1
    src, dst = g.edge_src.tolist(), g.edge_dst.tolist()
    for e in range(g.n_edges):
        assert nk[src[e]] == ek[e] >> 2 and nk[dst[e]] == ek[e] & mask, e
    print("ORACLE_OK", g.n_nodes, g.n_edges, flush=True)
"""
_ROUTES = {"default": {}, "s2_sort": {"KATOME_S2_GROUP_SORT": "0"}, "edge_sort": {"KATOME_EDGE_HALF_SORT": "0"}}
_MERGE_CASES = ["crowded_1", "crowded_1023", "crowded_1024", "crowded_1025", "crowded_12293", "cg_only", "k11", "k13"]
_GROUPED = "ordered per group in the merge"


@pytest.fixture(scope="module")
def routes():
    """route -> (case -> its MG row, case -> the trace lines of its build, stdout); the three processes run side by side"""
    env = dict(os.environ, KATOME_SORTED_COUNT="2", KATOME_LC_TRACE="1")
    for name in ("KATOME_S2_GROUP_SORT", "KATOME_EDGE_HALF_SORT", "KATOME_S2_GROUP_CAP"):
        env.pop(name, None)
    procs = {name: subprocess.Popen([sys.executable, "-c", _MERGE_SCRIPT, ROOT, "oracle" if name == "default" else "-"], env=dict(env, **extra),
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for name, extra in _ROUTES.items()}
    res = {}
    try:
        for name, p in procs.items():
            out, err = p.communicate(timeout=300)
            assert p.returncode == 0, (name, out[-1500:], err[-3000:])
            rows = {line.split()[1]: line.split() for line in out.splitlines() if line.startswith("MG ")}
            trace, case = {}, None
            for line in err.splitlines():
                if line.startswith("CASE "):
                    case = line.split()[1]
                    trace[case] = []
                elif case is not None:
                    trace[case].append(line)
            res[name] = (rows, trace, out)
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    return res


def _s2_line(trace_lines):
    for line in trace_lines:
        m = re.search(r"\[half sort\] S2: (\d+) keys, largest group (\d+): (.*)", line)
        if m:
            return int(m.group(2)), m.group(3)
    return None


@pytest.mark.parametrize("case", _MERGE_CASES)
def test_merge_every_route_gives_the_same_arrays(routes, case):
    rows = routes["default"][0]
    assert case in rows
    for name in _ROUTES:
        assert routes[name][0].get(case) == rows[case], (name, case)
    # the default route did order this build's S2 per group in the merge, and the other two did not
    s2 = _s2_line(routes["default"][1][case])
    assert s2 is not None and _GROUPED in s2[1], routes["default"][1][case]
    if case.startswith("crowded_"):
        assert _s2_line(routes["s2_sort"][1][case]) is None and _s2_line(routes["edge_sort"][1][case]) is None


@pytest.mark.parametrize("n", [1023, 1024, 1025, 12 * 1024 + 5])
def test_merge_group_sizes_are_what_the_case_means(routes, n):
    s2 = _s2_line(routes["default"][1]["crowded_%d" % n])
    assert s2 is not None and s2[0] == n, s2


def test_merge_empty_first_and_last_group(routes):
    """reads of C and G alone: no edge in group 0 or group 65535, on either strand"""
    row = routes["default"][0]["cg_only"]
    assert 0 < int(row[4]) and int(row[5]) < 0xFFFF, row
    # ... and the crowded builds do fill group 0
    assert int(routes["default"][0]["crowded_1025"][4]) == 0


def test_merge_a_crowded_group_equals_the_oracle(routes):
    assert "ORACLE_OK" in routes["default"][2]
