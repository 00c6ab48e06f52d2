"""The tile seams of the GFA writers.  Every GFA text is written in tiles of 8192 output bytes by one shared loop per kind of text
(write_line_tile of katome_amd/csrc/gfa_image.h for the H/S/L texts, write_piece_tile of gfa_path_lines.h for the P lines), so an
error at a seam would break every text at once.  Each text here -- katome_dev_gfa_arrays, its coverage form, the numbered part (S
part with and without header, L part), the strand-merged text at both key widths, the two path texts -- is hand-made so that a chosen
byte lies at a chosen place relative to byte 8192: a line's start at 8192 + d for d = -16 .. 16, the text's end on a tile's last
and first byte, an S line's tag tail, an S line's "S\\t<name>\\t" and a P line's head across the seam.
A case is moved into place by `pad`: more bases on the first, long segment, more digits in the first links' numbers, or in the first
pieces' ids.  Where the boundary lies is asserted on the MODEL's text before the device is asked; the bytes and the offset arrays are
then compared with the models by the helpers of each text's own test."""
import re

import numpy as np
import pytest

import coverage_model
import dist_gfa_model as dm
import gfa_model
import gfa_paths_model
import gfa_strand_paths_model
import gfa_strands_model as sm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE = 8192
K = 11
SWEEP = range(-16, 17)


def test_the_tile_is_what_the_cases_assume():
    from test_gpu_coverage import _tile_bytes
    assert _tile_bytes() == TILE == dm.TILE


def fit(text, where, target):
    """-> the pad at which where(text(pad)) == target"""
    pad = 0
    for _ in range(8):
        at = where(text(pad))
        if at == target:
            return pad
        pad += target - at
    raise AssertionError("no pad puts the boundary at %d" % target)


def line_starts(text):
    out, at = [], 0
    for ln in text.split(b"\n")[:-1]:
        out.append(at)
        at += len(ln) + 1
    return out


# ---- the S/L texts: a long first segment, a handful of k-base segments, their links -----------------------------------------------
class Text:
    """text(pad): the model's bytes; check(pad): the device's bytes and arrays against the model.  The first S line is the long one"""
    links_follow = True                                # the L lines lie in the same text

    def second_segment(self, text):
        return [at for at in line_starts(text) if text[at:at + 2] == b"S\t"][1]

    def first_link(self, text):
        return [at for at in line_starts(text) if text[at:at + 2] == b"L\t"][0]

    def tail_of_first_segment(self, text):
        at = text.index(b"\tLN:i:")
        return at, text.index(b"\n", at) + 1

    def head_of_second_segment(self, text):
        at = self.second_segment(text)
        return at, text.index(b"\t", at + 2) + 1


class Gfa(Text):
    def __init__(self):
        rng = np.random.default_rng(41)
        self.core = "".join(rng.choice(list("ACGT"), 17000))
        self.short = ["".join(rng.choice(list("ACGT"), K)) for _ in range(4)]
        self.weight = [1, 2 ** 32 - 1, 7, 99999, 3]
        self.src, self.dst = list(range(5)), list(range(1, 6))

    def seqs(self, pad):
        return [self.core[:8000 + pad]] + self.short

    def text(self, pad):
        seqs = self.seqs(pad)
        return gfa_model.gfa_text(K, self.src, self.dst, self.weight, [len(s) - K + 1 for s in seqs], seqs)[0]

    def check(self, pad):
        from test_gpu_gfa import check_arrays
        check_arrays(K, 6, self.src, self.dst, self.weight, self.seqs(pad))


class Coverage(Gfa):
    def cov(self, seqs):
        mn, mx = [1, 2 ** 32 - 1, 0, 12345, 3], [2 ** 32 - 1, 2 ** 32 - 1, 7, 10 ** 9, 4]
        return [w * (len(s) - K + 1) for w, s in zip(self.weight, seqs)], mn, mx

    def text(self, pad):
        seqs = self.seqs(pad)
        return coverage_model.gfa_coverage_text(K, self.src, self.dst, self.weight, [len(s) - K + 1 for s in seqs], seqs, *self.cov(seqs))[0]

    def check(self, pad):
        from test_gpu_coverage import check_arrays
        seqs = self.seqs(pad)
        check_arrays(K, 6, self.src, self.dst, self.weight, seqs, *self.cov(seqs))


class Part(Gfa):
    """the S part of a numbered part; its names cross from 19 to 20 digits"""
    links_follow = False
    first = 10 ** 19 - 2
    link_first, link_b = [0, 1, 3, 3, 4, 5], [7, 10 ** 19, 99, 2 ** 64 - 1, 0]

    def __init__(self, with_header):
        Gfa.__init__(self)
        self.with_header = with_header

    def parts(self, pad):
        seqs = self.seqs(pad)
        return dm.part_text(K, self.weight, [len(s) - K + 1 for s in seqs], seqs, self.first, self.with_header, self.link_first, self.link_b)

    def text(self, pad):
        return self.parts(pad)[0]

    def check(self, pad):
        from test_gpu_dist_gfa import _check_part
        _check_part(K, self.weight, self.seqs(pad), self.first, self.with_header, self.link_first, self.link_b)


class PartLinks(Part):
    """the L part of a numbered part: 400 links of five short segments; pad: more digits in the first links' second numbers"""
    def __init__(self):
        Part.__init__(self, 1)
        self.link_first = [0, 80, 160, 240, 320, 400]

    def seqs(self, pad):
        return self.short + self.short[:1]

    def parts(self, pad):
        assert 0 <= pad <= 19 * 400
        self.link_b = [10 ** min(19, max(0, pad - 19 * j)) for j in range(400)]
        return Part.parts(self, pad)

    def text(self, pad):
        return self.parts(pad)[1]

    def check(self, pad):
        self.parts(pad)
        Part.check(self, pad)

    def line(self, text):
        return line_starts(text)[240]


class Strands(Text):
    """edge 0 is the long segment and edge 5 its twin, edges 1 and 3 a short pair: the long S line carries rc / rw"""
    def __init__(self, k):
        from test_gpu_gfa_strands import Maker
        self.k = k
        m = Maker(k, np.random.default_rng(43 + k))
        while True:                                    # (the long segment ends in the same k-mer whatever its length)
            self.core, self.last = m.random(17000), m.random(k)
            if m.take(self.core[:k] + self.last):
                break
        self.short = [m.fresh(k) for _ in range(3)]
        self.weight = [1, 2 ** 32 - 1, 7, 99999, 3, 10 ** 9]
        self.src, self.dst = list(range(6)), list(range(1, 7))

    def seqs(self, pad):
        a, b, c = self.short
        s0 = self.core[:8000 + pad - self.k] + self.last
        return [s0, a, b, sm.revcomp(a), c, sm.revcomp(s0)]

    def text(self, pad):
        seqs = self.seqs(pad)
        text, names, _, _, twin = sm.strands_text(self.k, self.src, self.dst, self.weight, [len(s) - self.k + 1 for s in seqs], seqs)
        assert names == [0, 1, 2, 4] and twin[0] == 5 and b"\trc:i:5\trw:i:1000000000\n" in text
        return text

    def check(self, pad):
        from test_gpu_gfa_strands import check_arrays
        check_arrays(self.k, 7, self.src, self.dst, self.weight, self.seqs(pad))


TEXTS = {"gfa": Gfa, "coverage": Coverage, "part_header": lambda: Part(1), "part_no_header": lambda: Part(0), "strands_k3": lambda: Strands(3),
         "strands_k33": lambda: Strands(33)}


@pytest.fixture(scope="module", params=sorted(TEXTS))
def sl_text(request):
    return TEXTS[request.param]()


def test_a_line_starts_around_the_seam(sl_text):
    t = sl_text
    for where in [t.second_segment] + ([t.first_link] if t.links_follow else []):
        for d in SWEEP:
            pad = fit(t.text, where, TILE + d)
            assert TILE + d in line_starts(t.text(pad))
            t.check(pad)


def test_a_link_of_a_part_starts_around_the_seam():
    t = PartLinks()
    for d in SWEEP:
        pad = fit(t.text, t.line, TILE + d)
        assert line_starts(t.text(pad))[240] == TILE + d and t.text(pad)[TILE + d:TILE + d + 2] == b"L\t"
        t.check(pad)


@pytest.mark.parametrize("end", [2 * TILE, 2 * TILE + 1])
def test_the_text_ends_on_a_tiles_edge(sl_text, end):
    """2 * TILE bytes: the last byte is a tile's last; one more: a tile's first"""
    pad = fit(sl_text.text, len, end)
    assert len(sl_text.text(pad)) == end
    sl_text.check(pad)


@pytest.mark.parametrize("end", [2 * TILE, 2 * TILE + 1])
def test_the_links_of_a_part_end_on_a_tiles_edge(end):
    t = PartLinks()
    pad = fit(t.text, len, end)
    assert len(t.text(pad)) == end
    t.check(pad)


def _across(t, field):
    """the seam between every two neighbouring bytes of the field (some 8 places of a long one), asserted on the model's text"""
    lo, hi = field(t.text(0))
    n = 0
    for j in range(1, hi - lo, max(1, (hi - lo) // 8)):
        pad = fit(t.text, lambda text: field(text)[0] + j, TILE)
        lo2, hi2 = field(t.text(pad))
        assert lo2 < TILE < hi2 and lo2 + j == TILE                         # bytes of the field on both sides of the seam
        t.check(pad)
        n += 1
    return n


def test_a_tag_tail_lies_across_the_seam(sl_text):
    assert _across(sl_text, sl_text.tail_of_first_segment) >= 8
    lo, hi = sl_text.tail_of_first_segment(sl_text.text(0))
    assert sl_text.text(0)[lo:hi].startswith(b"\tLN:i:8000\tKC:i:") and sl_text.text(0)[hi - 1:hi] == b"\n"


def test_a_segments_name_lies_across_the_seam(sl_text):
    lo, hi = sl_text.head_of_second_segment(sl_text.text(0))
    assert re.fullmatch(rb"S\t\d+\t", sl_text.text(0)[lo:hi])
    assert _across(sl_text, sl_text.head_of_second_segment) >= 3


# ---- the path texts: one long run, a jump, then short runs -------------------------------------------------------------------------
class Paths:
    """1000 edges that all follow each other (one vertex) and edge 1000 on a vertex of its own.  Contig 0 is a run of 2600 pieces and,
    after a jump, the run "katome_0.1"; 300 contigs of one to three pieces follow.  pad: more digits in the first pieces' ids"""
    N, LONG = 1000, 2600
    src, dst = [0] * 1000 + [1], [0] * 1000 + [1]

    def pieces(self, pad):
        assert 0 <= pad <= 2 * self.LONG
        ids = [555 if 2 * j + 1 < pad else 55 if 2 * j < pad else 5 for j in range(self.LONG)]       # two more bytes, one more, none
        out = [ids[0] | gfa_paths_model.WHOLE] + ids[1:] + [self.N, self.N]
        for c in range(300):
            out += [(c * 7 % self.N) | gfa_paths_model.WHOLE] + [c % 10, 123][:c % 3]
        return out

    def model(self, pad):
        return gfa_paths_model.path_text(self.src, self.dst, self.pieces(pad))

    def text(self, pad):
        return self.model(pad)[0]

    def run(self, pad):
        from test_gpu_gfa_paths import run_arrays
        return run_arrays(self.src, self.dst, self.pieces(pad))[:5]

    def check(self, pad):
        want, want_off, want_contig, want_first, want_jumps = self.model(pad)
        text, counts, line_off, contig, first = self.run(pad)
        n, n_paths = len(want), len(want_contig)
        assert (counts["n_paths"], counts["n_jumps"], counts["text_bytes"]) == (n_paths, want_jumps, n) and want_jumps == 1
        assert bytes(text[:n]) == want
        assert not text[n:(n + 15) // 16 * 16].any() and (text[max((n + 15) // 16 * 16, 16):] == 0xFF).all()
        assert line_off[:n_paths + 1] == want_off and first[:n_paths + 1] == want_first and contig[:n_paths] == want_contig


class StrandPaths(Paths):
    """... over merged segments: edges 2i and 2i + 1 are twins, edge 1000 has none, so piece 5 reads "4-" and 555 "554-\""""
    twin = [i ^ 1 for i in range(1000)] + [-1]

    def model(self, pad):
        return gfa_strand_paths_model.path_text(self.src, self.dst, self.twin, self.pieces(pad))

    def run(self, pad):
        from test_gpu_gfa_strand_paths import run_arrays
        return run_arrays(self.src, self.dst, self.twin, self.pieces(pad))[:5]


@pytest.fixture(scope="module", params=["paths", "strand_paths"])
def path_text(request):
    return {"paths": Paths, "strand_paths": StrandPaths}[request.param]()


def test_a_path_line_starts_around_the_seam(path_text):
    t = path_text
    assert (b"4-," in t.text(0)) == isinstance(t, StrandPaths)
    for line in (1, 2):                                # the run after the jump, "P\tkatome_0.1\t"; the next contig, "P\tkatome_1\t"
        for d in SWEEP:
            pad = fit(t.text, lambda text: line_starts(text)[line], TILE + d)
            assert t.model(pad)[1][line] == TILE + d
            t.check(pad)


@pytest.mark.parametrize("end", [2 * TILE, 2 * TILE + 1])
def test_the_path_text_ends_on_a_tiles_edge(path_text, end):
    pad = fit(path_text.text, len, end)
    assert path_text.model(pad)[1][-1] == end
    path_text.check(pad)


def test_a_path_lines_head_lies_across_the_seam(path_text):
    t = path_text
    head = b"P\tkatome_0.1\t"
    for j in range(1, len(head)):
        pad = fit(t.text, lambda text: line_starts(text)[1] + j, TILE)
        want, off = t.model(pad)[:2]
        assert off[1] == TILE - j and want[off[1]:off[1] + len(head)] == head      # j bytes of the head in front of the seam, the rest behind
        t.check(pad)
