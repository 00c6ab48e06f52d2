"""A list-fed level of two-word records with its count in the key word (csrc/counted_key.h) against the same level with
plain keys and a weights array, through katome_dev_count_in_key: the records after the first and after the second partition pass,
unpacked, are equal array for array; the lists of distinct (key, count) are equal as sorted multisets and equal to a Python dictionary
sum of (oriented sub-window -> count); whole builds are equal across KATOME_COUNT_IN_KEY and equal to the oracle.

The switches are read once, so each setting runs in ONE child process of its own under a time limit, started once for the module:
  full      KATOME_LC_FULL=1: the counted form of lds_count_full_kernel counts the packed records (inputs this small are otherwise never
            offered to it), the salt word gives code 7 and goes the way back; and the builds with the switch on
  unpacked  KATOME_LC_FULL=0: every packed level is split into plain keys and weights before it is counted
  off       KATOME_LC_FULL=1 KATOME_COUNT_IN_KEY=0: the builds on the plain route
A child that ends any other way than with status 0 fails the tests, which start nothing more."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (tile_bases, sub_len, span, stride): C3's mid level; the narrowest and the widest sub-window that fit; one base too wide
C3 = (60, 36, 5, 6)
NARROW, WIDE, TOO_WIDE = (57, 33, 5, 6), (63, 39, 5, 6), (60, 40, 5, 5)
# list entries: 5, 4095, 4100 and 8195 records of 2048 to a sort tile -- a partial tile, one record short of two tiles, four records into
# a third, four tiles and three records; 2048 is no multiple of 5, so entries straddle the tile ends
ENTRIES = (1, 819, 820, 1639)

_SCRIPT = r"""
import ctypes as C, sys, hashlib, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii, int_to_kmer
from oracle import oracle as o
from katome_amd import _lib, device as kd
mode = sys.argv[2]; C3 = eval(sys.argv[3]); NARROW, WIDE, TOO_WIDE = eval(sys.argv[4]); ENTRIES = eval(sys.argv[5])
L = _lib.lib()
rng = np.random.default_rng(41)
SALT = 0x9E3779B97F4A7C15
M32 = (1 << 32) - 1

def rc_int(x, k):
    y = 0
    for _ in range(k):
        y = (y << 2) | (3 - (x & 3)); x >>= 2
    return y

def model(tiles, counts, form, rc):
    (tile_bases, sub, span, stride) = form
    mask = (1 << (2 * sub)) - 1
    want = {}
    for t, c in zip(tiles, counts):
        for q in range(span):
            w = (t >> (2 * (tile_bases - sub - q * stride))) & mask
            if rc:
                w = min(w, rc_int(w, sub))
            want[w] = (want.get(w, 0) + int(c)) & M32
    return want

def level(name, tiles, counts, form, rc, expect_packed=True):
    (tile_bases, sub, span, stride) = form
    n_tiles = len(tiles); n = n_tiles * span
    words = np.array([[t >> 64, t & ((1 << 64) - 1)] for t in tiles], dtype=np.uint64)
    d_tiles = torch.from_numpy(words.view(np.int64).reshape(-1).copy()).cuda()
    d_cnt = torch.from_numpy(np.array(counts, dtype=np.uint32).view(np.int32).copy()).cuda()
    got = []
    for packed in (1, 0):
        pk = [torch.zeros(n * 2, dtype=torch.int64, device="cuda") for _ in range(2)]
        pw = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        ok = torch.zeros(n * 2, dtype=torch.int64, device="cuda"); ow = torch.zeros(n, dtype=torch.int32, device="cuda")
        n_out = C.c_uint64(0); took = C.c_int(-1)
        st = L.katome_dev_count_in_key(0, kd._ptr(d_tiles), kd._ptr(d_cnt), n_tiles, tile_bases, sub, span, stride, rc, packed, kd._ptr(pk[0]), kd._ptr(pw[0]),
                                       kd._ptr(pk[1]), kd._ptr(pw[1]), kd._ptr(ok), kd._ptr(ow), C.byref(n_out), C.byref(took), kd._stream())
        assert st == 0, (name, packed, st, _lib.last_error())
        torch.cuda.synchronize()
        assert took.value == (1 if packed and expect_packed else 0), (name, packed, took.value)
        m = int(n_out.value)
        keys = ok.cpu().numpy().view(np.uint64).reshape(-1, 2)[:m]; w = ow.cpu().numpy().view(np.uint32)[:m]
        lst = sorted(((int(a) << 64) | int(b), int(c)) for (a, b), c in zip(keys, w))
        got.append((pk, pw, lst))
    for p in range(2):          # the passes are stable and deterministic: array for array
        assert torch.equal(got[0][0][p], got[1][0][p]), (name, "keys after pass", p + 1)
        assert torch.equal(got[0][1][p], got[1][1][p]), (name, "weights after pass", p + 1)
    assert int(got[0][1][1].to(torch.int64).bitwise_and(M32).sum().item()) == sum(int(c) for c in counts) * span, name
    want = sorted(model(tiles, counts, form, rc).items())
    assert got[0][2] == got[1][2], (name, "packed against plain", len(got[0][2]), len(got[1][2]))
    assert got[0][2] == want, (name, "against the dictionary", len(got[0][2]), len(want))
    print("LV", name, n_tiles, n, len(want), flush=True)

def random_tiles(n, tile_bases):
    return [int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * tile_bases)) - 1) for _ in range(n)]

def some_counts(n):
    c = rng.integers(1, 1 << 20, size=n, dtype=np.uint64)
    c[rng.integers(0, n, size=max(n // 4, 1))] = 1
    c[rng.integers(0, n, size=max(n // 4, 1))] = 0xFFFF
    c[rng.integers(0, n, size=max(n // 4, 1))] = 0x10000
    return [int(v) for v in c]

print("LEVELS", file=sys.stderr, flush=True)
for rc in (1, 0):
    s = "rc" if rc else "one_strand"
    # C3's form: distinct random tiles at every size, and entries drawn from a pool of 40 tiles so that sub-windows repeat
    for n_ent in ENTRIES:
        level("c3_%s_%d" % (s, n_ent), random_tiles(n_ent, 60), some_counts(n_ent), C3, rc)
    pool = random_tiles(40, 60)
    tiles = [pool[i] for i in rng.integers(0, 40, size=1639)] + random_tiles(1, 60)
    level("c3_%s_repeats" % s, tiles, some_counts(1639) + [0xFFFFFFFF], C3, rc)          # (the full count on a tile met once)
    # one entry many times over: sums pass 2^16 and stay below 2^32
    level("c3_%s_one_entry" % s, random_tiles(1, 60) * 1639, [0xFFFF] * 1639, C3, rc)
    assert 1 << 16 < 0xFFFF * 1639 < 1 << 32
    # the width limits
    level("narrow_%s" % s, random_tiles(820, 57), some_counts(820), NARROW, rc)
    level("wide_%s" % s, random_tiles(820, 63), some_counts(820), WIDE, rc)
    level("too_wide_%s" % s, random_tiles(820, 60), some_counts(820), TOO_WIDE, rc, expect_packed=False)
    # poly-A (all words 0) and poly-T (all key bits set with one strand) among random tiles, and alone
    for form, tb in ((C3, 60), (NARROW, 57), (WIDE, 63)):
        poly = [0, (1 << (2 * tb)) - 1]
        level("poly_%s_%d" % (s, form[1]), poly * 3 + random_tiles(400, tb) + poly, some_counts(408), form, rc)
        level("poly_alone_%s_%d" % (s, form[1]), poly, [7, 0xFFFFFFFF - 7 if not rc else 9], form, rc)
    # the salt word: the last sub-window of a tile is its low 72 bits -- low word the salt, bits 64 .. 71 clear (it starts AAAA, its
    # reverse complement G: the forward cut is the canonical one)
    salted = [(t >> 72 << 72) | SALT for t in random_tiles(3, 60)]
    print("SALT", file=sys.stderr, flush=True)
    level("salt_%s" % s, random_tiles(815, 60) + salted + random_tiles(2, 60), some_counts(820), C3, rc)
    print("SALTED", file=sys.stderr, flush=True)

# whole builds: k = 31, both strands, 150 bp (big tiles, mid tiles of 36 bases, k-mers) and 101 bp, every level counted by sorting
for read_len in (150, 101):
    reads = o.synth_reads(31, 3000, read_len, 30000, 3e-3, 0)
    print("BUILD %d" % read_len, file=sys.stderr, flush=True)
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(31, True)
    b.count_reads(packed, len(reads), reads.shape[1], None, first_read=0)
    dg = b.finalize()
    arrays = [t.cpu().numpy() for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label)]
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    print("FR", read_len, dg.n_nodes, dg.n_edges, h.hexdigest(), flush=True)
    ref = o.build_ascii(reads, 31, True)
    got = sorted(zip((int_to_kmer(int(v), 31) for v in arrays[0].reshape(-1).view(np.uint64)), (int(w) for w in arrays[1])))
    assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges), (dg.n_nodes, dg.n_edges, ref.n_nodes, ref.n_edges)
    assert got == ref.multiset()
    print("ORACLE", read_len, "equal", flush=True)
    del dg
    b.close()
"""

_PACKED = "in the key word, no weights array"
_NO_ROOM = "plain keys and a weights array (no room in the key word)"
_SWITCHED_OFF = "plain keys and a weights array (KATOME_COUNT_IN_KEY=0)"
_UNPACKED = "records unpacked into plain keys and a weights array"
_FULL = "[lds count] whole keys in the slots (7 per thread): code "


def _child(mode, **env_extra):
    env = dict(os.environ, KATOME_LC_TRACE="1", KATOME_SORTED_COUNT="2")      # (the tile levels counted by sorting however small the input)
    for name in ("KATOME_COUNT_IN_KEY", "KATOME_LC_FULL", "KATOME_LC_FULL_PER", "KATOME_ENTRY_CUT", "KATOME_FUSED_RECORDS", "KATOME_FUSED_HIST"):
        env.pop(name, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", _SCRIPT, ROOT, mode, repr(C3), repr((NARROW, WIDE, TOO_WIDE)), repr(ENTRIES)], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, (mode, out.returncode, out.stdout[-1500:], out.stderr[-3000:])
    return out


@pytest.fixture(scope="module")
def runs():
    return {"full": _child("full", KATOME_LC_FULL="1"), "unpacked": _child("unpacked", KATOME_LC_FULL="0"),
            "off": _child("off", KATOME_LC_FULL="1", KATOME_COUNT_IN_KEY="0")}


def _rows(out, tag):
    return [line.split() for line in out.stdout.splitlines() if line.startswith(tag + " ")]


def _levels(out):
    return out.stderr.split("LEVELS")[1].split("BUILD")[0]


def test_every_level_equal_to_the_plain_route_and_to_the_dictionary(runs):
    """(the comparisons are the child's own asserts: it ended with status 0; here: every case ran, none was left out)"""
    per_strand = len(ENTRIES) + 2 + 3 + 6 + 1
    for out in runs.values():
        rows = _rows(out, "LV")
        assert len(rows) == 2 * per_strand, [r[1] for r in rows]
        assert {int(r[3]) for r in rows if r[1].startswith("c3_rc_") and r[1][6:].isdigit()} == {5, 4095, 4100, 8195}


def test_the_trace_says_which_form_the_records_took(runs):
    """two trace lines per level (the entry runs it packed, then plain): 40 bases never fit; the flag of the entry overrules the switch"""
    for name, out in runs.items():
        lv = _levels(out)
        n_levels = len(_rows(out, "LV"))
        assert lv.count("[count_in_key] ") - lv.count(_UNPACKED) == 2 * n_levels
        assert lv.count(_NO_ROOM) == 2 * 2                                   # (too_wide, both strands, both settings of the flag)
        assert lv.count(_PACKED) == n_levels - 2
        assert lv.count(_SWITCHED_OFF) == n_levels - 2                       # (the flag set to 0 reads as the switch)


def test_the_counted_kernel_counts_packed_records_and_the_salt_goes_the_way_back(runs):
    lv = _levels(runs["full"])
    n_packed = len(_rows(runs["full"], "LV")) - 2
    # KATOME_LC_FULL=1: every level, packed or plain, is counted by lds_count_full_kernel's two forms; a packed level is unpacked only
    # where that kernel met the salt word (code 7), which both forms do on the salted lists
    assert lv.count(_FULL + "0") + lv.count(_FULL + "7") == 2 * len(_rows(runs["full"], "LV"))
    salted = [part.split("SALTED")[0] for part in lv.split("SALT\n")[1:]]
    assert len(salted) == 2
    for part in salted:
        assert part.count(_FULL + "7") == 2 and part.count(_UNPACKED) == 1
    assert lv.count(_FULL + "7") == 4 and lv.count(_UNPACKED) == 2
    assert n_packed > 0


def test_without_the_full_kernel_every_packed_level_is_unpacked(runs):
    lv = _levels(runs["unpacked"])
    assert _FULL not in lv
    assert lv.count(_UNPACKED) == lv.count(_PACKED) == len(_rows(runs["unpacked"], "LV")) - 2


def test_builds_are_equal_across_the_switch_and_equal_to_the_oracle(runs):
    fr = {name: _rows(out, "FR") for name, out in runs.items()}
    assert len(fr["full"]) == 2 and fr["full"] == fr["off"] == fr["unpacked"]
    for out in runs.values():
        assert _rows(out, "ORACLE") == [["ORACLE", "150", "equal"], ["ORACLE", "101", "equal"]]
    # 150 bp: the mid level (36 bases) is the one list-fed level ordered by hash, and it takes the packed route unless switched off
    for name, said in (("full", _PACKED), ("unpacked", _PACKED), ("off", _SWITCHED_OFF)):
        build = runs[name].stderr.split("BUILD 150")[1].split("BUILD 101")[0]
        assert build.count("[count_in_key] ") - build.count(_UNPACKED) == 1 and said in build, build[-2000:]
    assert _UNPACKED in runs["unpacked"].stderr.split("BUILD 150")[1].split("BUILD 101")[0]
    assert _PACKED not in runs["off"].stderr.split("BUILD")[1]
