"""katome_amd/csrc/entry_cut.h -- the span records of a list entry cut together, one reverse complement per entry -- against the
per-record expression level_orientation(sub_window(tile, ., o)) of kmer_bits.h, bit for bit, and both against the rules on strings
written out here.  Runs without a GPU (tests/hostshim/entry_cut_host.cpp).

  window o      bases o * stride .. o * stride + sub_len - 1 of the tile
  both strands  the smaller of the window and its reverse complement; REP (odd one-word k): the one whose middle base is A or C
  one strand    the window
"""
import ctypes as C
import os
import random
import subprocess

import pytest

from helpers import int_to_words, kmer_to_int, revcomp_str

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostshim", "entry_cut_host.cpp")
HDRS = [os.path.join(ROOT, "katome_amd", "csrc", h) for h in ("entry_cut.h", "kmer_bits.h")]
u64p = C.POINTER(C.c_uint64)

# (tile bases, sub length, span, stride): the mid level and the k-mer level of k = 31, one-word tiles at k = 13, the widest two-word
# tile, and a two-word tile of exactly 64 bits
FORMS = [(60, 36, 5, 6), (36, 31, 6, 1), (18, 13, 6, 1), (63, 36, 4, 9), (32, 31, 2, 1)]


def words_for(bases):
    return 1 if 2 * bases <= 62 else 2 if 2 * bases <= 126 else 3          # (kmer_bits.h key_words_for_k)


def modes(sub_len):
    """(rc, rep): both strands and one, and REP where k is odd and fits one word"""
    out = [(1, 0), (0, 0)]
    if sub_len % 2 == 1 and words_for(sub_len) == 1:
        out += [(1, 1), (0, 1)]
    return out


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "hostshim", "libentry_cut_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.hs_entry_cut.restype = C.c_int
    lib.hs_entry_cut.argtypes = [u64p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, u64p, u64p]
    return lib


def expected(tile, sub_len, span, stride, rc, rep):
    out = []
    for o in range(span):
        w = tile[o * stride:o * stride + sub_len]
        if rc and rep:
            w = w if w[(sub_len - 1) // 2] in "AC" else revcomp_str(w)
        elif rc:
            w = min(w, revcomp_str(w))
        out.append(kmer_to_int(w))
    return out


def cut(shim, tile_int, form, rc, rep):
    """(records by entry, records by record), each a list of span integers"""
    bases, sub_len, span, stride = form
    nwt, nwk = words_for(bases), words_for(sub_len)
    t = (C.c_uint64 * nwt)(*int_to_words(tile_int, nwt))
    a, b = (C.c_uint64 * (span * nwk))(), (C.c_uint64 * (span * nwk))()
    assert shim.hs_entry_cut(t, nwt, nwk, sub_len, span, stride, rc, rep, a, b) == 0
    join = lambda v: [sum(int(v[o * nwk + q]) << (64 * (nwk - 1 - q)) for q in range(nwk)) for o in range(span)]
    return join(a), join(b)


def check(shim, tile, form, dirty_too=True):
    bases, sub_len, span, stride = form
    assert len(tile) == bases == sub_len + stride * (span - 1)
    clean = kmer_to_int(tile)
    nwt = words_for(bases)
    dirty = clean | (((1 << (64 * nwt)) - 1) & ~((1 << (2 * bases)) - 1))      # every bit of the top word above the tile set
    for rc, rep in modes(sub_len):
        want = expected(tile, sub_len, span, stride, rc, rep)
        for t in (clean, dirty) if dirty_too else (clean,):
            by_entry, by_record = cut(shim, t, form, rc, rep)
            assert by_record == want, (form, rc, rep, tile, hex(t))
            assert by_entry == by_record, (form, rc, rep, tile, hex(t))


@pytest.mark.parametrize("form", FORMS)
def test_random_tiles(shim, form):
    rng = random.Random(31 * form[0] + form[2])
    for _ in range(300):
        check(shim, "".join(rng.choice("ACGT") for _ in range(form[0])), form)


@pytest.mark.parametrize("form", FORMS)
def test_uniform_and_low_complexity_tiles(shim, form):
    bases = form[0]
    for tile in ("A" * bases, "T" * bases, "C" * bases, "G" * bases, ("AT" * bases)[:bases], ("TA" * bases)[:bases], ("ACGT" * bases)[:bases],
                 "T" * (bases - 1) + "A", "A" + "T" * (bases - 1), "A" * (bases // 2) + "T" * (bases - bases // 2)):
        check(shim, tile, form)


@pytest.mark.parametrize("form", FORMS)
def test_top_word_of_all_64_bits(shim, form):
    """the tile's top word with all its 64 bits set: check() runs every tile a second time with every bit above its 2 * bases set,
    and leading (and trailing) T's set every bit the tile itself has at that end -- the records must not change"""
    bases = form[0]
    rng = random.Random(64 + bases)
    for _ in range(50):
        tail = "".join(rng.choice("ACGT") for _ in range(bases - 8))
        check(shim, "TTTTTTTT" + tail, form)
        check(shim, tail + "TTTTTTTT", form)


@pytest.mark.parametrize("form", [f for f in FORMS if f[1] % 2 == 0])
def test_windows_that_are_their_own_reverse_complement(shim, form):
    """canonical's tie, at even sub length: every window in turn is made h + rc(h)"""
    bases, sub_len, span, stride = form
    rng = random.Random(7 * bases)
    for _ in range(40):
        for o in range(span):
            tile = [rng.choice("ACGT") for _ in range(bases)]
            h = "".join(rng.choice("ACGT") for _ in range(sub_len // 2))
            w = h + revcomp_str(h)
            assert w == revcomp_str(w)
            tile[o * stride:o * stride + sub_len] = w
            tile = "".join(tile)
            check(shim, tile, form)
            by_entry, _ = cut(shim, kmer_to_int(tile), form, 1, 0)
            assert by_entry[o] == kmer_to_int(w)
    # the whole tile its own reverse complement where its length is even: window o then mirrors window span - 1 - o
    if bases % 2 == 0:
        for _ in range(40):
            h = "".join(rng.choice("ACGT") for _ in range(bases // 2))
            tile = h + revcomp_str(h)
            check(shim, tile, form)
            by_entry, _ = cut(shim, kmer_to_int(tile), form, 1, 0)
            assert by_entry == by_entry[::-1]


def test_forms_that_do_not_exist_are_refused(shim):
    t = (C.c_uint64 * 3)(0, 0, 0)
    out = (C.c_uint64 * 16)()
    assert shim.hs_entry_cut(t, 2, 2, 36, 5, 6, 1, 1, out, out) == 1          # (REP is of one-word k-mers)
    assert shim.hs_entry_cut(t, 3, 2, 36, 5, 6, 1, 0, out, out) == 1
