"""tests/extract_model.py pinned before it judges a kernel: against helpers' string-level windows, against itself (tiles against
plain windows, reads of varying length against reads of one length, the column form against the string form) and on palindromes."""
import numpy as np
import pytest

import extract_model as em
from helpers import int_to_kmer, kmer_to_int, pack_reads_ascii, revcomp_str, windows_multiset, words_to_int

MARK = 1 << em.MARK_BIT


def _ints(rec):
    return [words_to_int(row) for row in rec]


def test_kmer_value_is_kmer_to_int():
    rng = np.random.default_rng(1)
    for length in (1, 2, 31, 32, 33, 63, 64, 95):
        s = em.random_seq(rng, length)
        assert em.kmer_value(s) == kmer_to_int(s)
    assert [em.words_for(b) for b in (1, 31, 32, 63, 64, 95)] == [1, 1, 2, 2, 3, 3]


def test_format_words_places_the_mark_in_word_0():
    v = kmer_to_int("T" * 32)            # 64 bits: word 0 of its two holds no base
    got = em.format_words([v, v, None], [False, True, False], 2)
    assert got.tolist() == [[0, 2 ** 64 - 1], [MARK, 2 ** 64 - 1], [2 ** 64 - 1, 2 ** 64 - 1]]
    got = em.format_words([5], [True], 1)
    assert got.tolist() == [[MARK | 5]]
    got = em.format_words([kmer_to_int("C" + "A" * 94)], [True], 3)
    assert got.tolist() == [[MARK | 1 << 60, 0, 0]]


@pytest.mark.parametrize("k,rc", [(5, False), (31, True), (32, True), (63, True)])
def test_fixed_records_are_the_windows_multiset(k, rc):
    rng = np.random.default_rng(k)
    reads = em.random_reads(rng, 7, 90)
    if k == 32:
        reads[0, :32] = np.frombuffer(b"ACGT" * 8, np.uint8)          # a palindrome among them
    want = windows_multiset(reads, k, rc)                               # both strands' windows when rc
    got = {}
    for v in _ints(em.fixed_records(reads, k, rc)):
        got[v] = got.get(v, 0) + 1
    seen = set()
    for km, cnt in want.items():
        r = revcomp_str(km)
        canon = min(kmer_to_int(km), kmer_to_int(r)) if rc else kmer_to_int(km)
        assert cnt == got[canon] * (2 if rc and r == km else 1), km
        seen.add(canon)
    assert seen == set(got)


@pytest.mark.parametrize("k,span,L", em.tile_cases(False) + em.tile_cases(True))
def test_tiles_and_remainder_cover_every_window_once(k, span, L):
    rng = np.random.default_rng(L)
    reads = em.random_reads(rng, 3, L)
    W = L - k + 1
    plain = _ints(em.fixed_records(reads, k, False))
    tiles = _ints(em.tile_records(reads, k, span, False))
    rest = _ints(em.remainder_records(reads, k, span, False))
    assert len(tiles) == 3 * (W // span) and len(rest) == 3 * (W % span)
    for r in range(3):
        covered = []
        for j in range(W // span):
            s = int_to_kmer(tiles[r * (W // span) + j], k + span - 1)
            assert s == bytes(reads[r, j * span:j * span + k + span - 1]).decode()
            covered += [kmer_to_int(s[i:i + k]) for i in range(span)]
        covered += rest[r * (W % span):(r + 1) * (W % span)]
        assert covered == plain[r * W:(r + 1) * W]


@pytest.mark.parametrize("k", [4, 6, 32])
def test_palindromes_carry_no_mark(k):
    s = "ACGT" * 8
    n_pal = 0
    for w in range(len(s) - k + 1):
        km = s[w:w + k]
        v, marked = em.window_record(s, w, k, True, True)
        r = revcomp_str(km)
        assert v == min(kmer_to_int(km), kmer_to_int(r))
        assert marked == (kmer_to_int(r) < kmer_to_int(km))
        if r == km:
            n_pal += 1
            assert not marked
    assert n_pal > 0
    rec = em.fixed_records(np.frombuffer(s.encode(), np.uint8)[None, :], k, True, mark=True)
    pal = np.array([s[w:w + k] == revcomp_str(s[w:w + k]) for w in range(len(s) - k + 1)])
    assert not (rec[pal, 0] & np.uint64(MARK)).any()


def test_a_window_whose_complement_is_smaller_is_marked():
    for length, nw in ((5, 1), (31, 1), (32, 2), (63, 2), (64, 3), (95, 3)):
        s = "T" * length                  # complement: all A
        assert em.window_record(s, 0, length, True, True) == (0, True)
        assert em.window_record(s, 0, length, True, False) == (0, False)
        assert em.window_record(s, 0, length, False, True) == (kmer_to_int(s), False)
        reads = np.frombuffer(s.encode(), np.uint8)[None, :]
        assert em.fixed_records(reads, length, True, mark=True).tolist() == [[MARK] + [0] * (nw - 1)]
        assert em.tile_records(reads, length - 1, 2, True, mark=True).tolist() == [[MARK] + [0] * (nw - 1)]
        assert em.tile_records(reads, length - 1, 2, True, mark=False).tolist() == [[0] * nw]
        a = "A" * length                  # the smaller strand already
        assert em.window_record(a, 0, length, True, True) == (0, False)


@pytest.mark.parametrize("k,span", [(12, 16), (31, 33), (32, 33), (63, 2)])
def test_var_functions_on_reads_of_one_length_equal_the_fixed_ones(k, span):
    rng = np.random.default_rng(k + span)
    L, n = k + 2 * span + 5, 6
    reads = em.random_reads(rng, n, L)
    seqs = [bytes(r).decode() for r in reads]
    W = L - k + 1
    for rc, mark in ((False, False), (True, False), (True, True)):
        assert np.array_equal(em.var_records(seqs, k, rc, mark), em.fixed_records(reads, k, rc, None, mark))
        t, tp, wp = em.var_tile_records(seqs, k, span, rc, mark)
        assert np.array_equal(t, em.tile_records(reads, k, span, rc, None, mark))
        assert tp.tolist() == [i * (W // span) for i in range(n + 1)] and wp.tolist() == [i * W for i in range(n + 1)]
        r, rp, wp = em.var_remainder_records(seqs, k, span, rc, mark)
        assert np.array_equal(r, em.remainder_records(reads, k, span, rc, None, mark))
        assert rp.tolist() == [i * (W % span) for i in range(n + 1)]


@pytest.mark.parametrize("k,span,L", [(5, 3, 40), (31, 23, 100), (31, 23, 261), (32, 33, 130), (63, 33, 160)])
def test_column_form_equals_string_form(k, span, L):
    rng = np.random.default_rng(L)
    reads = em.random_reads(rng, 9, L)
    reads[4] = np.frombuffer(("ACGT" * L)[:L].encode(), np.uint8)
    skip = np.zeros(9, np.uint8)
    skip[[0, 5]] = 1
    for rc, mark, sk in ((False, False, None), (True, False, skip), (True, True, None), (True, True, skip)):
        for f, args in ((em.fixed_records, (k,)), (em.tile_records, (k, span)), (em.remainder_records, (k, span))):
            assert np.array_equal(f(reads, *args, rc, sk, mark, fast=True), f(reads, *args, rc, sk, mark))
            assert np.array_equal(em.with_skipped(f(reads, *args, rc, None, mark), skip), f(reads, *args, rc, skip, mark))


def test_packers():
    rng = np.random.default_rng(3)
    for L in (8, 9, 10, 11):
        reads = em.random_reads(rng, 5, L)
        clean = pack_reads_ascii(reads)
        skip = np.array([0, 1, 0, 0, 0], np.uint8)
        noisy = em.pack_fixed(reads, rng, skip).reshape(5, -1)
        keep = np.uint8((0xFF << (2 * ((-L) % 4))) & 0xFF)
        assert np.array_equal(noisy[skip == 0] & np.array([0xFF] * (clean.shape[1] - 1) + [keep], np.uint8),
                              clean[skip == 0])
        seqs = [bytes(r).decode() for r in reads]
        packed, off, lens = em.pack_var(seqs)
        assert np.array_equal(packed, clean.reshape(-1)) and lens.tolist() == [L] * 5
        assert off.tolist() == [i * clean.shape[1] for i in range(6)]
    packed, off, lens = em.pack_var(["ACGTA", "TT", "GGGGCCCCA"])
    assert off.tolist() == [0, 2, 3, 6] and lens.tolist() == [5, 2, 9] and packed.size == 6
    assert packed.tolist() == [0b00011011, 0b00000000, 0b11110000, 0b10101010, 0b01010101, 0b00000000]
