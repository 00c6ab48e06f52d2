"""extract.hip record for record against tests/extract_model.py: every entry point, every kernel body, at the edges.

Every comparison is np.array_equal on the whole output.  Inputs are random bases; the pad bits of a read's last byte are random and
skipped reads are packed from random bytes; the output tensor is longer than needed, pre-filled with a sentinel, and whatever lies
past the last record must still hold it.

Which kernel body a case reaches, worked out from extract_fixed_t (stride = ceil(L/4), W = records per read of that call):
    LDS256   extract_fixed_kernel<NW, RC, 256>       stride <= 64 and 256*W < 65536, both pointers 16-byte aligned
    LDS64    extract_fixed_kernel<NW, RC, 64>        otherwise, while stride <= 256 and 64*W < 65536, both pointers aligned
    GENF     extract_general_kernel<.., FixedAddr>   stride > 256, or W >= 1024, or a pointer that is not 16-byte aligned
    VAR      extract_general_kernel<.., ArrayAddr>   the extract_var* entries, modes 0 / 1 / 2
NW is key_words_for_k of the record's bases: 1 up to 31, 2 up to 63, 3 up to 95.

    test                              case                                    entry               body    NW
    test_fixed_lds256                 k 31 / 30 L 150, k 31 L 31 (W = 1)      extract_fixed       LDS256  1     30: W = 121, odd record counts
                                      k 3 L 256 (W = 254, stride 64: the      extract_fixed       LDS256  1     i / W up to 65023; the library
                                        largest W and stride of this form)                                      takes no k below 3
                                      k 32 L 151, k 33 L 149, k 63 L 150,     extract_fixed       LDS256  2
                                        k 63 L 63 (W = 1)
    test_fixed_lds64                  k 31 L 300 (W 270, stride 75)           extract_fixed       LDS64   1
                                      k 3 L 1024 (W 1022, stride 256: the     extract_fixed       LDS64   1     i / W up to 65407
                                        largest W and stride of this form)
                                      k 40 L 1000                             extract_fixed       LDS64   2
    test_fixed_general_long_reads     L 1100 (stride 275), k 31 / k 63        extract_fixed       GENF    1 / 2
    test_fixed_general_first_read     k 31 L 150, first_read = 1 (38 bytes)   extract_fixed       GENF    1     aligned twin of the same buffer: LDS256
    test_fixed_general_out_offset     k 31 / k 63 L 150, out 8 bytes on       extract_fixed       GENF    1 / 2
                                      k 63 span 33 L 150, out 8 bytes on      tiles + remainder   GENF    3 / 2
    test_tiles (L <= 256, n = 257)    (k, span) (16, 16) 31 bases             tiles               LDS256  1     each of them: fixed, tiles and
                                      (31, 2) 32, (31, 33) 63                 tiles               LDS256  2     remainder; W % span 0, 1, span-1;
                                      (32, 33) 64, (63, 2) 64, (63, 33) 95    tiles               LDS256  3     L = k + span - 2: no tile
                                      their remainders (win0, W % span)       remainder           LDS256  1 / 2
    test_tiles (L > 256, n = 65)      the same spans                          tiles, remainder    LDS64   1 / 2 / 3
    test_second_trip                  k 31 L 261 span 23, n = 2048*64 + 65    remainder (1/read)  LDS64   1     tiles 2048, 2049: second trip
                                      k 31 L 100 span 23, n = 2048*256 + 257  remainder (1/read)  LDS256  1     tiles 2048, 2049, 2050
    test_var                          k 12 / 31; k 32 / 63                    extract_var         VAR 0   1; 2
                                      (12, 16) 27; (12, 33) 44, (31, 2) 32,   var_tiles           VAR 1   1; 2; 3
                                        (31, 33) 63; (32, 33) 64, (63, 2) 64,
                                        (63, 33) 95
                                      the same spans                          var_remainder       VAR 2   1 (k 12, 31); 2 (k 32, 63)
    test_mark_fixed                   k 30, k 32, (32, 33) 64 bases           fixed / tiles / rem LDS256, LDS64, GENF   1, 2, 3 each; mark on
    test_mark_var                     k 32, span 33                           var, tiles, rem     VAR 0 / 1 / 2         2, 3, 2; mark on
    mark off                          every other test here: bit 62 of word 0 is clear on every valid record
"""
import numpy as np
import pytest
import torch

import extract_model as em
from helpers import revcomp_str

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A5A5A5A5A
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
MARK = np.uint64(1 << em.MARK_BIT)
SLACK = 37            # sentinel words behind the records


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Out:
    """a sentinel-filled buffer; .view is what the entry gets as out= (16-byte aligned, or 8 bytes on)"""

    def __init__(self, n_words, offset):
        self.n, self.offset = n_words, 1 if offset else 0
        self.buf = torch.full((self.offset + n_words + SLACK,), SENT, dtype=torch.int64, device="cuda")
        self.view = self.buf[self.offset:]
        assert self.view.data_ptr() % 16 == 8 * self.offset

    def records(self, nw):
        """after the call: the records [n, nw]; everything around them is still the sentinel"""
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy().view(np.uint64)
        assert (host[:self.offset] == SENT).all() and (host[self.offset + self.n:] == SENT).all()
        return host[self.offset:self.offset + self.n].reshape(-1, nw)


def _same(got, want, mark):
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[0]
        raise AssertionError("first differing record %d word %d: %#x, model %#x (%d records differ)"
                             % (bad[0], bad[1], got[bad[0], bad[1]], want[bad[0], bad[1]], (got != want).any(axis=1).sum()))
    if not mark and got.size:
        valid = got[:, 0] != ONES
        assert not (got[valid, 0] & MARK).any()


def _skip_for(n, rng, extra=()):
    """the first and the last read of a trip of either LDS form, the last read, and a few others"""
    skip = np.zeros(n, np.uint8)
    idx = [0, 63, 64, 127, 255, 256, 511, n - 1] + list(extra) + list(rng.integers(0, n, size=3))
    skip[[i for i in idx if 0 <= i < n]] = 1
    return skip


class _Fixed:
    """n random reads of L bases on the device, clean and with a skip array (the skipped reads' bytes random)"""

    def __init__(self, seed, n, L, rows=(), extra_skip=()):
        rng = np.random.default_rng(seed)
        self.n, self.L = n, L
        self.reads = em.random_reads(rng, n, L)
        for r, s in rows:
            self.reads[r] = np.frombuffer(s.encode(), np.uint8)
        self.skip = _skip_for(n, rng, extra_skip)
        self.packed = _dev(em.pack_fixed(self.reads, rng))
        self.packed_skip = _dev(em.pack_fixed(self.reads, rng, self.skip))
        self.skip_t = _dev(self.skip)
        assert self.packed.data_ptr() % 16 == 0 and self.packed_skip.data_ptr() % 16 == 0

    def check(self, b, entry, span, rc, mark=False, offset=False, fast=False):
        """one entry with skip=None and with the skip array, against the model -> what it wrote with skip=None, [n, per read, nw]"""
        k, n, L = b.k, self.n, self.L
        W = L - k + 1
        if entry == "fixed":
            per, nw, want = W, b.nw, em.fixed_records(self.reads, k, rc, None, mark, fast)
        elif entry == "tiles":
            per, nw, want = W // span, b.tile_words(span), em.tile_records(self.reads, k, span, rc, None, mark, fast)
        else:
            per, nw, want = W % span, b.nw, em.remainder_records(self.reads, k, span, rc, None, mark, fast)
        assert want.shape == (n * per, nw)
        written = []
        for packed, skip_t, expect in ((self.packed, None, want), (self.packed_skip, self.skip_t, em.with_skipped(want, self.skip))):
            out = _Out(n * per * nw, offset)
            if entry == "fixed":
                got = b.extract_fixed(packed, n, L, skip_t, out=out.view)
            elif entry == "tiles":
                got = b.extract_tiles(packed, n, L, span, skip_t, out=out.view)
            else:
                got = b.extract_remainder(packed, n, L, span, skip_t, out=out.view)
            assert got.numel() == n * per * nw
            written.append(out.records(nw))
            _same(written[-1], expect, mark)
        return written[0].reshape(n, per, nw)


# ---- reads of one length ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 515])
@pytest.mark.parametrize("k,L", [(31, 150), (32, 151), (33, 149), (63, 150), (30, 150), (31, 31), (63, 63), (3, 256)])
def test_fixed_lds256(k, L, n, rc):
    """L mod 4 = 2, 3, 1 (n * stride is no multiple of 16 at the odd n); L == k: W = 1; k 3 L 256: W = 254, the largest this form takes"""
    from katome_amd import device as kd
    assert (L + 3) // 4 <= 64 and 256 * (L - k + 1) < 65536
    b = kd.Builder(k, rc)
    _Fixed(1000 * k + L + n, n, L).check(b, "fixed", 1, rc)
    b.close()


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 131])
@pytest.mark.parametrize("k,L", [(31, 300), (3, 1024), (40, 1000)])
def test_fixed_lds64(k, L, n, rc):
    from katome_amd import device as kd
    W = L - k + 1
    assert ((L + 3) // 4 > 64 or 256 * W >= 65536) and (L + 3) // 4 <= 256 and 64 * W < 65536
    b = kd.Builder(k, rc)
    _Fixed(1000 * k + L + n, n, L).check(b, "fixed", 1, rc)
    b.close()


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("k", [31, 63])
def test_fixed_general_long_reads(k, rc):
    from katome_amd import device as kd
    b = kd.Builder(k, rc)
    _Fixed(k, 5, 1100).check(b, "fixed", 1, rc)          # stride 275: no LDS form; 5350 records, 21 workgroups
    b.close()


@pytest.mark.parametrize("rc", [True, False])
def test_fixed_general_first_read(rc):
    """first_read = 1 moves the packed pointer by 38 bytes: the general form, over the buffer the aligned call reads in LDS"""
    from katome_amd import device as kd
    k, L, n = 31, 150, 258
    W = L - k + 1
    inp = _Fixed(7, n, L)
    b = kd.Builder(k, rc)
    want = em.fixed_records(inp.reads, k, rc)
    for packed, skip_t, expect in ((inp.packed, None, want), (inp.packed_skip, inp.skip_t, em.with_skipped(want, inp.skip))):
        whole, rest = _Out(n * W, False), _Out((n - 1) * W, False)
        b.extract_fixed(packed, n, L, skip_t, out=whole.view)
        b.extract_fixed(packed, n - 1, L, skip_t, out=rest.view, first_read=1)
        got_whole, got_rest = whole.records(1), rest.records(1)
        _same(got_whole, expect, False)
        _same(got_rest, expect[W:], False)
        assert np.array_equal(got_rest, got_whole[W:])
    b.close()


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("k,span", [(31, None), (63, None), (63, 33)])
def test_fixed_general_out_offset(k, span, rc):
    """the 256-read shape with out= 8 bytes past a 16-byte boundary: no 16-byte stores, so the general form"""
    from katome_amd import device as kd
    b = kd.Builder(k, rc)
    inp = _Fixed(k, 257, 150)
    inp.check(b, "fixed", 1, rc, offset=True)
    if span:
        inp.check(b, "tiles", span, rc, offset=True)
        inp.check(b, "remainder", span, rc, offset=True)
    b.close()


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("k,span,L", em.tile_cases(False) + em.tile_cases(True))
def test_tiles(k, span, L, rc):
    from katome_amd import device as kd
    n = 257 if L <= 256 else 65
    b = kd.Builder(k, rc)
    assert b.tile_words(span) == em.words_for(k + span - 1)
    inp = _Fixed(100 * k + span + L, n, L)
    for entry in ("fixed", "tiles", "remainder"):
        inp.check(b, entry, span, rc)          # (no whole tile, or nothing left over: the call returns without a launch)
    b.close()


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("L,trip", [(261, 64), (100, 256)])
def test_second_trip(L, trip, rc):
    """more than 2048 tiles: workgroups 0, 1 (and 2) go through the grid-stride loop twice, the second time over a short tile"""
    from katome_amd import device as kd
    k, span = 31, 23
    n = 2048 * trip + trip + 1
    assert (L - k + 1) % span == 1
    b = kd.Builder(k, rc)
    inp = _Fixed(L, n, L, extra_skip=(2048 * trip - 1, 2048 * trip, 2049 * trip - 1, 2049 * trip, 5 * trip + 1))
    inp.check(b, "remainder", span, rc, fast=True)
    b.close()


# ---- reads of varying length --------------------------------------------------------------------------------------------------------
def _var_seqs(rng, k, span, mode, layout, extra=()):
    """bulk: about 300 reads of k .. 400 bases and one of 5000; reads that give no record in this mode first, last, alone in the
    middle and three in a row"""
    if layout == "single":
        return [em.random_seq(rng, k + 3 * span)]           # 3 * span + 1 windows
    seqs = [em.random_seq(rng, int(x)) for x in rng.integers(k, 401, size=300)]
    seqs.insert(150, em.random_seq(rng, 5000))
    seqs[40:40] = list(extra)
    if mode == 1:
        none = lambda: em.random_seq(rng, k + int(rng.integers(0, span - 1)))            # fewer windows than span
    elif mode == 2:
        none = lambda: em.random_seq(rng, k - 1 + span * int(rng.integers(1, 5)))        # nothing after the last whole tile
    else:
        return seqs
    seqs[100:100] = [none()]
    seqs[200:200] = [none(), none(), none()]
    return [none()] + seqs + [none()]


def _check_var(b, seqs, span, mode, rc, mark, rng):
    k = b.k
    packed_h, off_h, len_h = em.pack_var(seqs, rng)
    assert packed_h.size == off_h[-1]                      # the buffer ends with the last read's last byte
    packed, off, lens = _dev(packed_h), _dev(off_h), _dev(len_h)
    if mode == 0:
        want, nw = em.var_records(seqs, k, rc, mark), b.nw
        wpref_h = pref_h = em.window_prefix(seqs, k)
    elif mode == 1:
        (want, pref_h, wpref_h), nw = em.var_tile_records(seqs, k, span, rc, mark), b.tile_words(span)
    else:
        (want, pref_h, wpref_h), nw = em.var_remainder_records(seqs, k, span, rc, mark), b.nw
    assert want.shape == (pref_h[-1], nw)
    pref, wpref = _dev(pref_h), _dev(wpref_h)
    out = _Out(want.size, False)
    if mode == 0:
        b.extract_var(packed, off, lens, wpref, int(wpref_h[-1]), out=out.view)
    elif mode == 1:
        b.extract_var_tiles(packed, off, lens, pref, wpref, int(pref_h[-1]), int(wpref_h[-1]), span, out=out.view)
    else:
        b.extract_var_remainder(packed, off, lens, pref, wpref, int(pref_h[-1]), int(wpref_h[-1]), span, out=out.view)
    got = out.records(nw)               # (synchronises: the prefix tensors are alive until here)
    del pref, wpref
    _same(got, want, mark)
    return got, want, pref_h


VAR_SPANS = [(12, 16), (12, 33), (31, 2), (31, 33), (32, 33), (63, 2), (63, 33)]


@pytest.mark.parametrize("layout", ["bulk", "single"])
@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("k,span,mode", [(k, 1, 0) for k in (12, 31, 32, 63)] + [(k, s, m) for m in (1, 2) for k, s in VAR_SPANS])
def test_var(k, span, mode, rc, layout):
    from katome_amd import device as kd
    rng = np.random.default_rng(1000 * k + 10 * span + mode)
    b = kd.Builder(k, rc)
    seqs = _var_seqs(rng, k, span, mode, layout)
    _, want, pref = _check_var(b, seqs, span, mode, rc, False, rng)
    if layout == "bulk" and mode:
        ties = np.flatnonzero(np.diff(pref) == 0)
        assert {0, len(seqs) - 1} <= set(ties) and (np.diff(ties) == 1).sum() >= 2 and want.shape[0] > 0
    b.close()


# ---- the orientation mark of first-seen builders -------------------------------------------------------------------------------------
def _palindromic(s, length, starts):
    return np.array([s[w:w + length] == revcomp_str(s[w:w + length]) for w in starts], dtype=bool)


@pytest.mark.parametrize("body,L,n,offset", [("lds256", 150, 257, False), ("lds64", 300, 65, False), ("general", 150, 257, True)])
@pytest.mark.parametrize("k,span", [(30, None), (32, None), (32, 33)])
def test_mark_fixed(k, span, body, L, n, offset):
    """first-seen builder with rc: bit 62 of word 0 exactly where the complement is strictly smaller; palindromes stay clear"""
    from katome_amd import device as kd
    pal = ("ACGT" * L)[:L]
    inp = _Fixed(k + L, n, L, rows=[(2, pal)])
    b = kd.Builder(k, True, first_seen_order=True)
    W = L - k + 1
    if span is None:
        got = inp.check(b, "fixed", 1, True, mark=True, offset=offset)
        where = _palindromic(pal, k, range(W))
    else:
        inp.check(b, "remainder", span, True, mark=True, offset=offset)
        got = inp.check(b, "tiles", span, True, mark=True, offset=offset)
        where = _palindromic(pal, k + span - 1, range(0, (W // span) * span, span))
    assert where.any() and not (got[2, where, 0] & MARK).any() and (got[:, :, 0] & MARK).any()
    b.close()
    # neither rc without first-seen order nor first-seen order without rc marks anything
    for bb, rc in ((kd.Builder(k, True), True), (kd.Builder(k, False, first_seen_order=True), False)):
        inp.check(bb, "tiles" if span else "fixed", span or 1, rc, mark=False, offset=offset)
        bb.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_mark_var(mode):
    from katome_amd import device as kd
    k, span = 32, 33
    rng = np.random.default_rng(mode)
    pal = "ACGT" * 60
    seqs = _var_seqs(rng, k, span, mode, "bulk", extra=[pal])
    b = kd.Builder(k, True, first_seen_order=True)
    got, want, pref = _check_var(b, seqs, span, mode, True, True, rng)
    at = seqs.index(pal)
    mine = got[pref[at]:pref[at + 1]]
    W = len(pal) - k + 1
    starts = range(W) if mode == 0 else range(0, (W // span) * span, span) if mode == 1 else range((W // span) * span, W)
    where = _palindromic(pal, k + span - 1 if mode == 1 else k, starts)
    assert len(mine) == len(where) and where.any() and not (mine[where, 0] & MARK).any()
    assert (got[:, 0] & MARK).any()
    b.close()
    for bb, rc in ((kd.Builder(k, True), True), (kd.Builder(k, False, first_seen_order=True), False)):
        _check_var(bb, seqs, span, mode, rc, False, rng)
        bb.close()


# ---- refusals and empties: no kernel runs, nothing is written -------------------------------------------------------------------------
def _untouched(out):
    torch.cuda.synchronize()
    assert (out.buf.cpu().numpy().view(np.uint64) == SENT).all()


def test_refusals():
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    inp = _Fixed(1, 4, 100)
    out = _Out(4096, False)
    b = kd.Builder(31, True)
    with pytest.raises(KatomePanic) as e:
        b.extract_fixed(inp.packed, 4, 30, out=out.view)
    assert e.value.name == "E_SHORT_READ"
    b.close()
    b = kd.Builder(63, True)
    with pytest.raises(KatomePanic) as e:
        b.extract_tiles(inp.packed, 4, 100, 34, out=out.view)           # 96 bases
    assert e.value.name == "E_ARG"
    seqs = ["ACGT" * 20, "TTGCA" * 20]
    packed_h, off_h, len_h = em.pack_var(seqs)
    pref = _dev(em.window_prefix(seqs, 63))
    with pytest.raises(KatomePanic) as e:
        b.extract_var_tiles(_dev(packed_h), _dev(off_h), _dev(len_h), pref, pref, int(pref[-1]), int(pref[-1]), 1, out=out.view)
    assert e.value.name == "E_ARG"
    b.close()
    _untouched(out)


def test_empties():
    from katome_amd import device as kd
    inp = _Fixed(2, 4, 100)
    out = _Out(4096, False)
    b = kd.Builder(31, True)
    assert b.extract_fixed(inp.packed, 0, 100, out=out.view).numel() == 0
    assert b.extract_tiles(inp.packed, 0, 100, 7, out=out.view).numel() == 0
    assert b.extract_remainder(inp.packed, 4, 100, 7, out=out.view).numel() == 0       # 70 windows: ten whole tiles
    assert b.extract_remainder(inp.packed, 4, 100, 7, inp.skip_t, out=out.view).numel() == 0
    assert b.extract_tiles(inp.packed, 4, 62, 33, out=out.view).numel() == 0                # 32 windows: no whole tile
    b.close()
    _untouched(out)
