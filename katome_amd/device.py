"""Device-resident driver over the C ABI: PyTorch supplies device memory, streams and
torch.distributed (plumbing); every kernel is in katome_amd/lib/libkatome_gpu.so.

Used by bench.py (inputs resident in HBM before the timed region); the multi-GPU bindings are in katome_amd/shard.py.  Mirrors the steps of `Build::create` (reference builder.rs:142-165 ->
pt_graph.rs:277-315,172-198,333-345): extract -> insert -> finalize.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from .build import ContigsStats, KatomePanic, collection_stats, make_settings


def _check(status):
    if status != 0:
        raise KatomePanic(status, _lib.last_error())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _ViewOwner:
    """owner of library memory that zero-copy views point into: close() while views are alive is put off until the last
    of them is gone (the library would hand the memory to the next build underneath them)"""

    _views = 0
    _close_pending = False

    def _retain_view(self):
        self._views += 1

    def _release_view(self):
        self._views -= 1
        if self._views == 0 and self._close_pending:
            self._close_pending = False
            self._destroy()

    def close(self):
        if self._views > 0:
            self._close_pending = True
        else:
            self._destroy()

    def _destroy(self):
        raise NotImplementedError


class _DevArray:
    """zero-copy view of library-owned device memory (kept alive by `owner`)"""

    def __init__(self, ptr, shape, typestr, owner):
        self.owner = owner
        if isinstance(owner, _ViewOwner):
            owner._retain_view()
            weakref.finalize(self, owner._release_view)
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def _view(ptr, shape, typestr, owner, device):
    n = 1
    for s in shape:
        n *= s
    if n == 0 or not ptr:
        dt = {"<i8": torch.int64, "<i4": torch.int32, "|u1": torch.uint8}[typestr]
        return torch.empty(shape, dtype=dt, device=device)
    return torch.as_tensor(_DevArray(ptr, shape, typestr, owner), device=device)


def record_words(k):
    return _lib.lib().katome_record_words(k)


class DeviceGraph:
    """finalized graph, arrays resident in HBM (int64/int32 views of the u64/u32 data)"""

    def __init__(self, dg, builder, device):
        self.n_nodes, self.n_edges = dg.n_nodes, dg.n_edges
        self.key_words, self.label_stride = dg.key_words, dg.label_stride
        nw, ne, nn = dg.key_words, dg.n_edges, dg.n_nodes
        self.edge_key = _view(dg.d_edge_key, (ne, nw), "<i8", builder, device)
        self.edge_weight = _view(dg.d_edge_weight, (ne,), "<i4", builder, device)
        self.edge_src = _view(dg.d_edge_src, (ne,), "<i8", builder, device)
        self.edge_dst = _view(dg.d_edge_dst, (ne,), "<i8", builder, device)
        self.edge_label = _view(dg.d_edge_label, (ne, dg.label_stride), "|u1", builder, device)
        self.node_key = _view(dg.d_node_key, (nn, nw), "<i8", builder, device)
        # first-seen index each edge had before remove_* re-numbered it (None while age == index)
        self.edge_age = _view(dg.d_edge_age, (ne,), "<i4", builder, device) if dg.d_edge_age else None


class DeviceContigs:
    """result of Builder.shrink(): merged edges with labels of any length (compress_edge format, edge i at
    edge_label[edge_label_off[i]:edge_label_off[i+1]]).  After shrink(coverage=True) also kmer_sum (int64 view of u64), kmer_min and
    kmer_max (int32 views of u32): per merged edge the sum, smallest and largest k-mer count of the input edges on its path.  The
    library drops them at the builder's next shrink of any kind; from then on the attributes raise instead of handing out views"""

    def __init__(self, dc, builder, device, cov=None):
        self.n_nodes, self.n_edges, self.label_bytes, self.key_words = dc.n_nodes, dc.n_edges, dc.label_bytes, dc.key_words
        ne, nn, nw = dc.n_edges, dc.n_nodes, dc.key_words
        self.edge_src = _view(dc.d_edge_src, (ne,), "<i8", builder, device)
        self.edge_dst = _view(dc.d_edge_dst, (ne,), "<i8", builder, device)
        self.edge_weight = _view(dc.d_edge_weight, (ne,), "<i4", builder, device)
        self.edge_kmers = _view(dc.d_edge_kmers, (ne,), "<i4", builder, device)
        self.edge_label_off = _view(dc.d_edge_label_off, (ne + 1,), "<i8", builder, device)
        self.edge_label = _view(dc.d_edge_label, (dc.label_bytes,), "|u1", builder, device)
        self.node_key = _view(dc.d_node_key, (nn, nw), "<i8", builder, device)
        self._dc, self._builder = dc, builder
        self.has_coverage = cov is not None
        self._shrink_serial = getattr(builder, "_shrink_serial", 0)
        if cov is not None:
            self._cov = (_view(cov.d_kmer_sum, (ne,), "<i8", builder, device), _view(cov.d_kmer_min, (ne,), "<i4", builder, device),
                         _view(cov.d_kmer_max, (ne,), "<i4", builder, device))

    def _coverage(self, j):
        if not self.has_coverage:
            raise AttributeError("these contigs were shrunk without coverage: Builder.shrink(coverage=True)")
        if self._shrink_serial != self._builder._shrink_serial:
            raise ValueError("the builder has shrunk again since: this result's coverage was dropped")
        return self._cov[j]

    kmer_sum = property(lambda self: self._coverage(0))
    kmer_min = property(lambda self: self._coverage(1))
    kmer_max = property(lambda self: self._coverage(2))

    def sequences(self):
        """host: every merged edge decoded to its ACGT string (compress.rs:283-293 decompress_edge)"""
        off = self.edge_label_off.cpu().numpy()
        lab = self.edge_label.cpu().numpy()
        out = []
        for i in range(self.n_edges):
            b = lab[off[i]:off[i + 1]]
            pad = int(b[0])
            bases = "".join("ACGT"[(int(x) >> s) & 3] for x in b[1:] for s in (6, 4, 2, 0))
            out.append(bases[:len(bases) - pad])
        return out


    def text(self, layout="plain"):
        """every merged edge's whole label as text, one contig per edge, written on the device (katome_dev_contigs_text) ->
        DeviceAssembly; valid for the builder's last shrink() only"""
        da = _lib.DevAssembly()
        _check(_lib.lib().katome_dev_contigs_text(self._builder._h, C.byref(self._dc), LAYOUTS[layout], C.byref(da), _stream()))
        return DeviceAssembly(da, self._builder, self._builder.tdev)

    def gfa(self, merge_strands=False, coverage=False):
        """the shrunk graph as GFA 1, written on the device (katome_dev_contigs_gfa; include/katome_gpu.h has the format) ->
        DeviceGfa; valid for the builder's last shrink() only, and until the next gfa().  merge_strands: strand twins as one
        segment with +/- links (katome_dev_contigs_gfa_strands) -> DeviceGfaStrands, valid until the next gfa(merge_strands=True).
        coverage: KC is the sum of the path's k-mer counts and every S line ends in mn / mx (katome_dev_contigs_gfa_coverage);
        needs contigs of shrink(coverage=True) and does not combine with merge_strands"""
        if coverage:
            if merge_strands:
                raise ValueError("gfa: coverage=True does not combine with merge_strands=True (the bidirected writer has no coverage form)")
            if not self.has_coverage:
                raise ValueError("gfa: coverage=True needs the contigs of Builder.shrink(coverage=True)")
            dg = _lib.DevGfa()
            _check(_lib.lib().katome_dev_contigs_gfa_coverage(self._builder._h, C.byref(self._dc), C.byref(dg), _stream()))
            return DeviceGfa(dg.n_segments, dg.n_links, dg.text_bytes, _view(dg.d_text, (dg.text_bytes,), "|u1", self._builder, self._builder.tdev),
                             _view(dg.d_segment_off, (dg.n_segments,), "<i8", self._builder, self._builder.tdev),
                             _view(dg.d_link_first, (dg.n_segments + 1,), "<i8", self._builder, self._builder.tdev))
        if merge_strands:
            d, b = _lib.DevGfaStrands(), self._builder
            _check(_lib.lib().katome_dev_contigs_gfa_strands(b._h, C.byref(self._dc), C.byref(d), _stream()))
            v = lambda p, n: _view(p, (n,), "<i8", b, b.tdev)
            return DeviceGfaStrands(d.n_segments, d.n_links, d.text_bytes, _view(d.d_text, (d.text_bytes,), "|u1", b, b.tdev), v(d.d_segment_off, d.n_segments),
                                    v(d.d_link_first, d.n_segments + 1), v(d.d_segment_name, d.n_segments), v(d.d_edge_twin, self.n_edges), d.n_unpaired,
                                    d.n_self_twins)
        dg = _lib.DevGfa()
        _check(_lib.lib().katome_dev_contigs_gfa(self._builder._h, C.byref(self._dc), C.byref(dg), _stream()))
        return DeviceGfa(dg.n_segments, dg.n_links, dg.text_bytes, _view(dg.d_text, (dg.text_bytes,), "|u1", self._builder, self._builder.tdev),
                         _view(dg.d_segment_off, (dg.n_segments,), "<i8", self._builder, self._builder.tdev),
                         _view(dg.d_link_first, (dg.n_segments + 1,), "<i8", self._builder, self._builder.tdev))


class DeviceGfa:
    """a GFA 1 text in HBM: text (uint8, text_bytes of them) is the file; segment_off[i] = offset of segment i's first base;
    the L lines of segment a are lines link_first[a] .. link_first[a + 1] of the L region"""

    def __init__(self, n_segments, n_links, text_bytes, text, segment_off, link_first):
        self.n_segments, self.n_links, self.text_bytes = n_segments, n_links, text_bytes
        self.text, self.segment_off, self.link_first = text, segment_off, link_first

    def bytes(self):
        """host: the file's bytes"""
        return bytes(self.text.cpu().numpy())


class DeviceGfaStrands(DeviceGfa):
    """a GFA 1 text with strand twins merged: S line s is merged edge segment_name[s] (segment_off[s]: its first base), the L lines
    whose first segment it is are lines link_first[s] .. link_first[s + 1] of the L region; edge_twin[i] = the merged edge that is
    edge i's reverse complement, -1 for none"""

    def __init__(self, n_segments, n_links, text_bytes, text, segment_off, link_first, segment_name, edge_twin, n_unpaired, n_self_twins):
        super().__init__(n_segments, n_links, text_bytes, text, segment_off, link_first)
        self.segment_name, self.edge_twin, self.n_unpaired, self.n_self_twins = segment_name, edge_twin, n_unpaired, n_self_twins


class DeviceGfaPaths(DeviceGfa):
    """the GFA of an assembly in HBM (katome_dev_collapse_gfa): text / segment_off / link_first as in DeviceGfa for the collapse's
    shrunk graph, then the contigs as P lines in path_text (uint8, path_bytes of them; on the device it starts at text_bytes
    rounded up to 16).  Path j is the line at path_line_off[j] of path_text, a run of contig path_contig[j] whose first piece is
    piece path_first_piece[j]; n_jumps = n_paths - n_contigs: the seams inside contigs that no L line covers"""

    def __init__(self, n_segments, n_links, text_bytes, text, segment_off, link_first, n_paths, n_jumps, path_bytes, path_text, path_line_off,
                 path_contig, path_first_piece):
        super().__init__(n_segments, n_links, text_bytes, text, segment_off, link_first)
        self.n_paths, self.n_jumps, self.path_bytes, self.path_text = n_paths, n_jumps, path_bytes, path_text
        self.path_line_off, self.path_contig, self.path_first_piece = path_line_off, path_contig, path_first_piece

    def bytes(self):
        """host: the file's bytes, the two parts back to back"""
        return bytes(self.text.cpu().numpy()) + bytes(self.path_text.cpu().numpy())


def unique_paths(path_mirror):
    """the paths that stay when every double-stranded molecule keeps one: those with no mirror (-1, or 2^64 - 1 as unsigned) or
    with mirror(j) >= j -> list of path indices.  This is the per-PATH rule: where a sequence occurs more than once it keeps an
    irregular subset of the copies.  The rule for CONTIGS, which keeps one strand with all its copies, is
    Builder.collapse_unique()'s (include/katome_gpu.h, katome_dev_collapse_unique)"""
    return [j for j, q in enumerate(int(x) for x in path_mirror) if q < 0 or q >= j]


class DeviceGfaStrandPaths(DeviceGfaStrands):
    """the bidirected GFA of an assembly in HBM (katome_dev_collapse_gfa_strands): text and the segment / link / twin arrays as in
    DeviceGfaStrands for the collapse's shrunk graph, then the contigs as P lines over the merged segments in path_text (the
    fields of DeviceGfaPaths; a piece reads <rep><o>).  path_mirror[j]: the smallest path that spells the same molecule from its
    other end, -1 for none; n_mirrored paths have one, n_self_mirror are their own"""

    def __init__(self, strands, n_edges, n_paths, n_jumps, path_bytes, path_text, path_line_off, path_contig, path_first_piece, n_mirrored, n_self_mirror,
                 path_mirror):
        super().__init__(*strands)
        self.n_edges, self.n_paths, self.n_jumps, self.path_bytes, self.path_text = n_edges, n_paths, n_jumps, path_bytes, path_text
        self.path_line_off, self.path_contig, self.path_first_piece = path_line_off, path_contig, path_first_piece
        self.n_mirrored, self.n_self_mirror, self.path_mirror = n_mirrored, n_self_mirror, path_mirror

    def bytes(self):
        """host: the file's bytes, the two parts back to back"""
        return bytes(self.text.cpu().numpy()) + bytes(self.path_text.cpu().numpy())

    def unique_paths(self):
        """the indices j with no mirror or mirror(j) >= j: one path per molecule"""
        return unique_paths(self.path_mirror.cpu().tolist())


LAYOUTS = {"plain": 0, "fasta": 1}


class DeviceAssembly:
    """contigs as text in HBM: contig i is text[contig_off[i]:contig_off[i] + contig_len[i]]; layout "plain": the contigs back
    to back, "fasta": text[:text_bytes] is byte for byte what Contigs::save_to_file writes (asm/mod.rs:57-72)"""

    def __init__(self, da, owner, device, stats=None):
        self.n_contigs, self.text_bytes = da.n_contigs, da.text_bytes
        self.layout = {v: k for k, v in LAYOUTS.items()}[da.layout]
        self.contig_off = _view(da.d_contig_off, (da.n_contigs,), "<i8", owner, device)
        self.contig_len = _view(da.d_contig_len, (da.n_contigs,), "<i4", owner, device)
        self.text = _view(da.d_text, (da.text_bytes,), "|u1", owner, device)
        self.collapse_stats = stats              # the walk's counters (Builder.collapse())
        self.n_pieces = stats["n_pieces"] if stats else da.n_contigs

    def lengths(self):
        return [int(x) & 0xFFFFFFFF for x in self.contig_len.cpu().tolist()]

    def contigs(self):
        """host: the contigs as a list of str, in order"""
        raw = bytes(self.text.cpu().numpy())
        return [raw[o:o + n].decode() for o, n in zip(self.contig_off.cpu().tolist(), self.lengths())]

    def contig_stats(self, original_genome_length):
        """Contigs::stats (stats/contigs.rs:31-89) of these contigs"""
        from .build import contig_stats
        return contig_stats(self.lengths(), original_genome_length)

    @property
    def stats(self):
        return self.collapse_stats


DEPTH_ENCODINGS = {"packed": 0, "ascii": 1}
DEPTH_ABSENT, DEPTH_INVALID, DEPTH_REVERSE = -1, -2, -(1 << 63)       # the per-window values as the int64 views show them


def _depth_flags(either_strand, windows, edge_hits):
    return (1 if either_strand else 0) | (2 if windows else 0) | (4 if edge_hits else 0)


class DeviceDepth:
    """result of Builder.depth() (katome_dev_depth, which has the definitions): per sequence seq_present, seq_invalid, seq_sum
    (int64 views of u64), seq_min, seq_max (int32 views of u32: -1 is all ones) and seq_window_off [n_seqs + 1]; the totals; with
    windows=True window_edge [n_windows] (int64 view: DEPTH_ABSENT, DEPTH_INVALID, or the edge's index, negative where
    DEPTH_REVERSE is set), with edge_hits=True edge_hits [n_edges]; otherwise None.  Valid until the builder's next depth() or close()"""

    def __init__(self, d, owner, device):
        for f in ("n_seqs", "n_windows", "n_present", "n_invalid", "n_edges", "n_edges_hit", "weight_sum"):
            setattr(self, f, int(getattr(d, f)))
        v = lambda p, n, t="<i8": _view(p, (n,), t, owner, device)
        self.seq_present, self.seq_invalid, self.seq_sum = v(d.d_seq_present, d.n_seqs), v(d.d_seq_invalid, d.n_seqs), v(d.d_seq_sum, d.n_seqs)
        self.seq_min, self.seq_max = v(d.d_seq_min, d.n_seqs, "<i4"), v(d.d_seq_max, d.n_seqs, "<i4")
        self.seq_window_off = v(d.d_seq_window_off, d.n_seqs + 1)
        self.window_edge = v(d.d_window_edge, d.n_windows) if d.d_window_edge else None
        self.edge_hits = v(d.d_edge_hits, d.n_edges, "<i4") if d.d_edge_hits else None

    @staticmethod
    def of_text(builder, assembly, either_strand=False, windows=False, edge_hits=False):
        """the contigs of a DeviceAssembly (collapse() or contigs_text(), either layout, of any builder on this device) queried
        against `builder`'s graph through contig_off / contig_len, in ASCII, without a copy of the text"""
        return builder.depth(assembly.text, assembly.contig_off, assembly.contig_len, "ascii", either_strand, windows, edge_hits)


class DeviceUniqueAssembly:
    """the strand-unique assembly in HBM (katome_dev_collapse_unique, which has the definitions): contig_mirror[c] = the smallest
    contig that spells c's molecule from its other end by pieces, -1 for none (n_mirrored have one, n_self_mirror are their own);
    the kept contigs -- one strand per molecule with all its copies -- are kept_name (ascending, their numbers in collapse()'s
    result), kept contig i is text[kept_off[i]:kept_off[i] + kept_len[i]]; layout "fasta": text is the kept records of
    collapse("fasta")'s text, byte for byte"""

    def __init__(self, n_contigs, n_mirrored, n_self_mirror, contig_mirror, n_kept, text_bytes, layout, kept_name, kept_off, kept_len, text):
        self.n_contigs, self.n_mirrored, self.n_self_mirror, self.contig_mirror = n_contigs, n_mirrored, n_self_mirror, contig_mirror
        self.n_kept, self.text_bytes, self.layout = n_kept, text_bytes, layout
        self.kept_name, self.kept_off, self.kept_len, self.text = kept_name, kept_off, kept_len, text

    def lengths(self):
        return [int(x) & 0xFFFFFFFF for x in self.kept_len.cpu().tolist()]

    def bytes(self):
        """host: the text's bytes"""
        return bytes(self.text.cpu().numpy()[:self.text_bytes])

    def contigs(self):
        """host: the kept contigs as a list of str, in order"""
        raw = self.bytes()
        return [raw[o:o + n].decode() for o, n in zip(self.kept_off.cpu().tolist(), self.lengths())]


class Builder(_ViewOwner):
    """one GPU's share of a build"""

    def __init__(self, k, reverse_complement, device=0, table_slots_hint=0, first_seen_order=False):
        self.k, self.rc, self.device = k, bool(reverse_complement), device
        self.nw = record_words(k)
        self._settings = make_settings(k, reverse_complement=reverse_complement, device=device,
                                       table_slots_hint=table_slots_hint, first_seen_order=first_seen_order)
        self._h = C.c_void_p()
        _check(_lib.lib().katome_builder_create(C.byref(self._settings), C.byref(self._h)))
        self.tdev = torch.device("cuda", device)

    # ---- per-phase HIP-event timing (on the stream the kernels run on) ---------------------------
    def profile(self, enable=True):
        _check(_lib.lib().katome_builder_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        """{phase: (total_ms, launches, elements processed)} since the last read; synchronises.  Entries "k:<kernel>" are
        single kernels timed launch by launch inside the phases (elements: keys of a pass, slots of a scan ...)"""
        L = _lib.lib()
        n = L.katome_phase_count()
        ms, cnt, work = (C.c_double * n)(), (C.c_uint64 * n)(), (C.c_uint64 * n)()
        _check(L.katome_builder_profile_read_work(self._h, ms, cnt, work))
        return {L.katome_phase_name(i).decode(): (ms[i], int(cnt[i]), int(work[i])) for i in range(n) if cnt[i]}

    def counts(self):
        """{distinct_tiles, tile_slots, distinct_kmers, kmer_slots} of the last edges()/finalize()"""
        out = (C.c_uint64 * 8)()
        _check(_lib.lib().katome_builder_counts(self._h, out))
        return dict(distinct_tiles=out[0], tile_slots=out[1], distinct_kmers=out[2], kmer_slots=out[3],
                    distinct_mid_tiles=out[4], mid_tile_slots=out[5], span=out[6], mid_span=out[7])

    def _destroy(self):
        if self._h:
            _lib.lib().katome_builder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    # ---- extraction (compress_kmer[_with_rev_compl] over read.windows(K)) -----------------------
    def extract_fixed(self, packed, n_reads, read_len, skip=None, out=None, first_read=0):
        stride = (read_len + 3) // 4
        n_rec = n_reads * (read_len - self.k + 1) if read_len >= self.k else 0
        if out is None:
            out = torch.empty(max(n_rec, 1) * self.nw, dtype=torch.int64, device=self.tdev)
        assert out.numel() >= n_rec * self.nw
        p = C.c_void_p(packed.data_ptr() + first_read * stride)
        sk = C.c_void_p(skip.data_ptr() + first_read) if skip is not None else None
        _check(_lib.lib().katome_dev_extract_fixed(self._h, p, n_reads, read_len, sk, _ptr(out), _stream()))
        return out[:n_rec * self.nw]

    # ---- tiled counting: (k+span-1)-mers covering `span` consecutive windows ---------------------------
    def tile_span(self, read_len):
        return _lib.lib().katome_tile_span(self.k, read_len)

    def tile_words(self, span):
        return _lib.lib().katome_tile_words(self.k, span)

    def extract_tiles(self, packed, n_reads, read_len, span, skip=None, out=None, first_read=0):
        stride = (read_len + 3) // 4
        nwt = self.tile_words(span)
        n_rec = n_reads * ((read_len - self.k + 1) // span)
        if out is None:
            out = torch.empty(max(n_rec, 1) * nwt, dtype=torch.int64, device=self.tdev)
        assert out.numel() >= n_rec * nwt
        p = C.c_void_p(packed.data_ptr() + first_read * stride)
        sk = C.c_void_p(skip.data_ptr() + first_read) if skip is not None else None
        _check(_lib.lib().katome_dev_extract_tiles(self._h, p, n_reads, read_len, span, sk, _ptr(out), _stream()))
        return out[:n_rec * nwt]

    def tile_plan(self, read_len, max_tile_words=3):
        """(span, tiles per read, single windows left over per read); span 1 = count every window on its own"""
        sp, t, r = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.lib().katome_tile_plan_limited(self.k, read_len, max_tile_words, C.byref(sp), C.byref(t), C.byref(r))
        return sp.value, t.value, r.value

    def extract_remainder(self, packed, n_reads, read_len, span, skip=None, out=None, first_read=0):
        """the windows of every read that come after its last whole tile, as plain k-mer records"""
        stride = (read_len + 3) // 4
        W = read_len - self.k + 1
        n_rec = n_reads * (W % span)
        if out is None:
            out = torch.empty(max(n_rec, 1) * self.nw, dtype=torch.int64, device=self.tdev)
        assert out.numel() >= n_rec * self.nw
        p = C.c_void_p(packed.data_ptr() + first_read * stride)
        sk = C.c_void_p(skip.data_ptr() + first_read) if skip is not None else None
        _check(_lib.lib().katome_dev_extract_remainder(self._h, p, n_reads, read_len, span, sk, _ptr(out), _stream()))
        return out[:n_rec * self.nw]

    def count_reads(self, packed, n_reads, read_len, skip=None, first_read=0):
        """one batch through the library's plan: tiles (+ left-over windows), or every window on its own"""
        span, tiles, rest = self.tile_plan(read_len)
        if span > 1:
            self.count_tiles(packed, n_reads, read_len, span, skip, first_read=first_read)
            if rest:
                self.insert(self.extract_remainder(packed, n_reads, read_len, span, skip, first_read=first_read))
        else:
            self.insert(self.extract_fixed(packed, n_reads, read_len, skip, first_read=first_read))

    def count_tiles(self, packed, n_reads, read_len, span, skip=None, first_read=0):
        """extract_tiles + insert_tiles without a record buffer of the caller's (the records are made where the builder keeps them)"""
        stride = (read_len + 3) // 4
        p = C.c_void_p(packed.data_ptr() + first_read * stride)
        sk = C.c_void_p(skip.data_ptr() + first_read) if skip is not None else None
        _check(_lib.lib().katome_dev_count_tiles(self._h, p, n_reads, read_len, span, sk, _stream()))

    def insert_tiles(self, records, span):
        n = records.numel() // self.tile_words(span)
        _check(_lib.lib().katome_dev_insert_tiles(self._h, _ptr(records), n, span, _stream()))

    def expand_tiles(self):
        """(k-mer keys [n*nw] int64 view, weights [n] int32 view) of this builder's tiles; the tile table is released"""
        pk, pw, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(_lib.lib().katome_dev_expand_tiles(self._h, C.byref(pk), C.byref(pw), C.byref(n), _stream()))
        return (_view(pk.value, (n.value * self.nw,), "<i8", self, self.tdev),
                _view(pw.value, (n.value,), "<i4", self, self.tdev))

    def extract_var(self, packed, byte_off, lens, win_prefix, total_windows, out=None):
        n_reads = lens.numel()
        if out is None:
            out = torch.empty(max(total_windows, 1) * self.nw, dtype=torch.int64, device=self.tdev)
        _check(_lib.lib().katome_dev_extract_var(self._h, _ptr(packed), packed.numel(), _ptr(byte_off), _ptr(lens),
                                                 _ptr(win_prefix), n_reads, total_windows, _ptr(out), _stream()))
        return out[:total_windows * self.nw]

    def extract_var_tiles(self, packed, byte_off, lens, tile_prefix, win_prefix, total_tiles, total_windows, span, out=None):
        """the whole tiles of `span` windows from the front of every read (tile_prefix: tiles before each read of the batch)"""
        nwt = self.tile_words(span)
        if out is None:
            out = torch.empty(max(total_tiles, 1) * nwt, dtype=torch.int64, device=self.tdev)
        assert out.numel() >= total_tiles * nwt
        _check(_lib.lib().katome_dev_extract_var_tiles(self._h, _ptr(packed), packed.numel(), _ptr(byte_off), _ptr(lens), _ptr(tile_prefix),
                                                       _ptr(win_prefix), lens.numel(), total_tiles, total_windows, span, _ptr(out), _stream()))
        return out[:total_tiles * nwt]

    def extract_var_remainder(self, packed, byte_off, lens, rest_prefix, win_prefix, total_rest, total_windows, span, out=None):
        """the windows of every read after its last whole tile (rest_prefix: such windows before each read of the batch)"""
        if out is None:
            out = torch.empty(max(total_rest, 1) * self.nw, dtype=torch.int64, device=self.tdev)
        assert out.numel() >= total_rest * self.nw
        _check(_lib.lib().katome_dev_extract_var_remainder(self._h, _ptr(packed), packed.numel(), _ptr(byte_off), _ptr(lens), _ptr(rest_prefix),
                                                           _ptr(win_prefix), lens.numel(), total_rest, total_windows, span, _ptr(out), _stream()))
        return out[:total_rest * self.nw]

    def count_var_reads(self, packed, byte_off, lens, span=None, batch_windows=None):
        """Reads of varying length through the library's plan, as katome_build_files feeds them: batch by batch (of at most
        `batch_windows` windows; None: one batch) the whole tiles of `span` windows, then the windows left over -- or every window on
        its own (span 1).  packed: the reads' bases, 4 per byte, every read starting on a byte (byte_off [n + 1] int64, lens [n]
        int32, both on the device); span None: tile_span_for_lengths' choice.  None of the reads may be shorter than k."""
        k = self.k
        h_len = lens.cpu().numpy().astype(np.int64)
        assert h_len.size == 0 or h_len.min() >= k
        if span is None:
            span = tile_span_for_lengths(k, h_len)
        W = h_len - k + 1
        cum = np.cumsum(W)
        r0, n = 0, int(h_len.size)
        while r0 < n:
            # (as many reads as stay within batch_windows, one at least)
            r1 = n if batch_windows is None else max(r0 + 1, int(np.searchsorted(cum, (cum[r0 - 1] if r0 else 0) + batch_windows, "right")))
            w = W[r0:r1]
            dev = lambda a: torch.from_numpy(np.concatenate(([0], np.cumsum(a))).astype(np.int64)).to(self.tdev)
            windows, boff, ln, pref = int(w.sum()), byte_off[r0:r1 + 1], lens[r0:r1], dev(w)
            if span > 1:
                tiles, rest = int((w // span).sum()), int((w % span).sum())
                tpref, rpref = dev(w // span), dev(w % span)         # (the insert reads the prefixes its extraction was given)
                if tiles:
                    self.insert_tiles(self.extract_var_tiles(packed, boff, ln, tpref, pref, tiles, windows, span), span)
                self.insert(self.extract_var_remainder(packed, boff, ln, rpref, pref, rest, windows, span))     # (also closes the batch)
            else:
                self.insert(self.extract_var(packed, boff, ln, pref, windows))
            torch.cuda.synchronize(self.tdev)          # (the prefixes are read by the kernels: they stay until the batch is through)
            r0 = r1

    # ---- routing for the multi-GPU exchange -----------------------------------------------------
    def partition(self, records, n_parts, key_words=None, values=None, core=None):
        """records grouped by owner rank (stable, invalid dropped); -> (records_out, counts[, values_out]).
        core=(shift_bits, bases): owner by the key's canonical core instead of the whole key (katome_dev_partition_core)"""
        nw = key_words or self.nw
        n = records.numel() // nw
        out = torch.empty_like(records)
        vout = torch.empty_like(values) if values is not None else None
        counts = (C.c_uint64 * n_parts)()
        if core is None:
            _check(_lib.lib().katome_dev_partition(self.device, _ptr(records), _ptr(values), n, nw, n_parts, _ptr(out), _ptr(vout),
                                                   counts, _stream()))
        else:
            _check(_lib.lib().katome_dev_partition_core(self.device, _ptr(records), _ptr(values), n, nw, core[0], core[1], n_parts,
                                                        _ptr(out), _ptr(vout), counts, _stream()))
        counts = [int(c) for c in counts]
        return (out, counts) if values is None else (out, counts, vout)

    # ---- add_single_edge_fastaq for a batch ------------------------------------------------------
    def insert(self, records, weights=None):
        n = records.numel() // self.nw
        if weights is None:
            _check(_lib.lib().katome_dev_insert(self._h, _ptr(records), n, _stream()))
        else:
            _check(_lib.lib().katome_dev_insert_weighted(self._h, _ptr(records), _ptr(weights), n, _stream()))

    def remove_weak_edges(self, threshold):
        """Clean::remove_weak_edges (pruner.rs:84-93).  Before finalize(): applied when the edges are read out (first-seen
        order: after the numbering, with petgraph's retain_edges / retain_nodes re-numbering).  On a finalized
        first-seen-order builder: applied now, same re-numbering; fetch the arrays again with graph()."""
        _check(_lib.lib().katome_dev_remove_weak_edges(self._h, threshold, _stream()))

    def standardize_contigs(self):
        """Standardizable::standardize_contigs (standardizer.rs:72-122) on the finalized graph, in place"""
        _check(_lib.lib().katome_dev_standardize_contigs(self._h, _stream()))

    def standardize_edges(self, original_genome_length, threshold):
        """Standardizable::standardize_edges (standardizer.rs:42-70): scale, round, remove_weak_edges(1)"""
        _check(_lib.lib().katome_dev_standardize_edges(self._h, original_genome_length, threshold, _stream()))

    _shrink_serial = 0

    def shrink(self, mode=None, coverage=False):
        """Shrinkable::shrink (shrinker.rs:165-209) of the finalized graph as it stands -> DeviceContigs.  mode "exact": the
        reference's own cuts and numbering, index for index (its traversal order on one host core, the bytes on the device);
        "fast": traversal-free, all on the device, this library's numbering; None: exact on a first-seen-order builder.
        `self.last_shrink_host_ms`: the sequential part of the last exact call.  coverage: the result also has kmer_sum, kmer_min
        and kmer_max per merged edge (katome_dev_shrink_coverage), accumulated by the same walk"""
        dc = _lib.DevContigs()
        host_ms = C.c_double(0)
        self._shrink_serial += 1
        if coverage:
            cov = _lib.DevCoverage()
            _check(_lib.lib().katome_dev_shrink_coverage(self._h, {None: 0, "auto": 0, "fast": 1, "exact": 2}[mode], C.byref(dc), C.byref(cov),
                                                         C.byref(host_ms), _stream()))
            self.last_shrink_host_ms = host_ms.value
            return DeviceContigs(dc, self, self.tdev, cov)
        _check(_lib.lib().katome_dev_shrink_mode(self._h, {None: 0, "auto": 0, "fast": 1, "exact": 2}[mode], C.byref(dc), C.byref(host_ms),
                                                 _stream()))
        self.last_shrink_host_ms = host_ms.value
        return DeviceContigs(dc, self, self.tdev)

    def collapse(self, layout="plain"):
        """Collapsable::collapse (collapser.rs:25-273) of the finalized graph as it stands -> DeviceAssembly: the exact shrink, the
        reference's walk on one host core (`self.last_collapse_host_ms`), the text written on the device.  The builder's graph
        is left as it is; the result is valid until the next collapse() or close()"""
        da, st = _lib.DevAssembly(), _lib.CollapseStats()
        _check(_lib.lib().katome_dev_collapse(self._h, LAYOUTS[layout], C.byref(da), C.byref(st), _stream()))
        stats = {f: getattr(st, f) for f, _ in _lib.CollapseStats._fields_}
        self.last_collapse_host_ms = st.host_ms
        return DeviceAssembly(da, self, self.tdev, stats)

    def collapse_gfa(self, merge_strands=False):
        """the GFA of the last collapse(): its shrunk graph as H, S and L lines and its contigs as P lines over those segments, one
        line per run of properly linked pieces (katome_dev_collapse_gfa; include/katome_gpu.h has the format) -> DeviceGfaPaths,
        valid until the next collapse_gfa() or close().  The results of collapse() and of gfa() stay valid.  merge_strands: strand
        twins as one segment, +/- in the links and in the paths, and every path's mirror (katome_dev_collapse_gfa_strands) ->
        DeviceGfaStrandPaths, valid until the next collapse_gfa(merge_strands=True); neither call touches the other's result"""
        if merge_strands:
            d = _lib.DevGfaStrandPaths()
            _check(_lib.lib().katome_dev_collapse_gfa_strands(self._h, C.byref(d), _stream()))
            v = lambda p, n: _view(p, (n,), "<i8", self, self.tdev)
            u = lambda p, n: _view(p, (n,), "|u1", self, self.tdev)
            strands = (d.n_segments, d.n_links, d.text_bytes, u(d.d_text, d.text_bytes), v(d.d_segment_off, d.n_segments), v(d.d_link_first, d.n_segments + 1),
                       v(d.d_segment_name, d.n_segments), v(d.d_edge_twin, d.n_edges), d.n_unpaired, d.n_self_twins)
            return DeviceGfaStrandPaths(strands, d.n_edges, d.n_paths, d.n_jumps, d.path_bytes, u(d.d_path_text, d.path_bytes), v(d.d_path_line_off, d.n_paths + 1),
                                        v(d.d_path_contig, d.n_paths), v(d.d_path_first_piece, d.n_paths + 1), d.n_mirrored, d.n_self_mirror,
                                        v(d.d_path_mirror, d.n_paths))
        d = _lib.DevGfaPaths()
        _check(_lib.lib().katome_dev_collapse_gfa(self._h, C.byref(d), _stream()))
        v = lambda p, n: _view(p, (n,), "<i8", self, self.tdev)
        return DeviceGfaPaths(d.n_segments, d.n_links, d.text_bytes, _view(d.d_text, (d.text_bytes,), "|u1", self, self.tdev), v(d.d_segment_off, d.n_segments),
                              v(d.d_link_first, d.n_segments + 1), d.n_paths, d.n_jumps, d.path_bytes, _view(d.d_path_text, (d.path_bytes,), "|u1", self, self.tdev),
                              v(d.d_path_line_off, d.n_paths + 1), v(d.d_path_contig, d.n_paths), v(d.d_path_first_piece, d.n_paths + 1))

    def collapse_unique(self, layout="fasta"):
        """the strand-unique form of the last collapse(), whatever layout that used: every contig's mirror by piece sequence, the
        kept set and its text under the contigs' original numbers (katome_dev_collapse_unique; include/katome_gpu.h has the
        definitions) -> DeviceUniqueAssembly, valid until the next collapse_unique() or close().  The results of collapse(),
        collapse_gfa() and gfa() stay valid"""
        d = _lib.DevUniqueAssembly()
        _check(_lib.lib().katome_dev_collapse_unique(self._h, LAYOUTS[layout], C.byref(d), _stream()))
        v = lambda p, n, t="<i8": _view(p, (n,), t, self, self.tdev)
        return DeviceUniqueAssembly(d.n_contigs, d.n_mirrored, d.n_self_mirror, v(d.d_contig_mirror, d.n_contigs), d.n_kept, d.text_bytes, layout,
                                    v(d.d_kept_name, d.n_kept), v(d.d_kept_off, d.n_kept), v(d.d_kept_len, d.n_kept, "<i4"), v(d.d_text, d.text_bytes, "|u1"))

    def graph(self):
        """the finalized graph as it stands (after remove_dead_paths / remove_weak_edges)"""
        dg = _lib.DevGraph()
        _check(_lib.lib().katome_dev_current_graph(self._h, C.byref(dg)))
        return DeviceGraph(dg, self, self.tdev)

    def stats(self):
        """Stats<CollectionStats>::stats (stats/collections.rs:137-168) of the finalized graph as it stands, computed on the
        device (katome_dev_graph_stats) -> build.CollectionStats"""
        st = _lib.Stats()
        _check(_lib.lib().katome_dev_graph_stats(self._h, C.byref(st), _stream()))
        return collection_stats(st, capacity=(st.node_count, st.edge_count))

    def depth(self, seq, byte_off, lens, encoding="packed", either_strand=False, windows=False, edge_hits=False):
        """every window of every sequence looked up among the edges of the finalized graph as it stands (katome_dev_depth) ->
        DeviceDepth.  seq: uint8 on the device ("packed": 4 bases per byte, every sequence starting on a byte; "ascii": a byte per
        base, only upper-case ACGT are bases); byte_off int64 [n] (more entries are ignored), lens int32 [n], both on the device"""
        d = _lib.DevDepth()
        n = lens.numel()
        assert byte_off.numel() >= n and byte_off.dtype == torch.int64 and lens.dtype == torch.int32 and seq.dtype == torch.uint8
        _check(_lib.lib().katome_dev_depth(self._h, DEPTH_ENCODINGS[encoding], _depth_flags(either_strand, windows, edge_hits), _ptr(seq), seq.numel(),
                                           _ptr(byte_off), _ptr(lens), n, C.byref(d), _stream()))
        return DeviceDepth(d, self, self.tdev)

    def depth_index_bytes(self):
        """device bytes of the lookup index depth() keeps between calls (0: none is kept)"""
        return int(_lib.lib().katome_dev_depth_index_bytes(self._h))

    def weight_spectrum(self, n_bins):
        """np.uint64[n_bins]: edges of weight w at [w], those of weight >= n_bins - 1 in the last bin (katome_dev_weight_spectrum)"""
        bins = np.zeros(max(int(n_bins), 0), np.uint64)
        _check(_lib.lib().katome_dev_weight_spectrum(self._h, bins.ctypes.data_as(_lib.u64p), n_bins, _stream()))
        return bins

    def table_count(self):
        out = C.c_uint64()
        _check(_lib.lib().katome_dev_table_count(self._h, C.byref(out), _stream()))
        return out.value

    # ---- PtGraph::create post-pass -----------------------------------------------------------------
    def edges(self):
        """sorted distinct oriented edges of this builder's table: (keys [n, nw] int64 view, weights [n] int32 view)"""
        pk, pw, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(_lib.lib().katome_dev_edges(self._h, C.byref(pk), C.byref(pw), C.byref(n), _stream()))
        return (_view(pk.value, (n.value, self.nw), "<i8", self, self.tdev),
                _view(pw.value, (n.value,), "<i4", self, self.tdev))

    def finalize(self):
        dg = _lib.DevGraph()
        _check(_lib.lib().katome_dev_finalize(self._h, C.byref(dg), _stream()))
        return DeviceGraph(dg, self, self.tdev)

    def remove_dead_paths(self):
        """Prunable::remove_dead_paths (pruner.rs:36-82) on the finalized first-seen-ordered graph, in place
        -> (DeviceGraph, stats dict)"""
        dg, st = _lib.DevGraph(), _lib.PruneStats()
        _check(_lib.lib().katome_dev_remove_dead_paths(self._h, C.byref(dg), C.byref(st), _stream()))
        return DeviceGraph(dg, self, self.tdev), {f: getattr(st, f) for f, _ in _lib.PruneStats._fields_}


def tile_span_for_lengths(k, lens):
    """one tile span for reads of several lengths (none shorter than k), the one katome_build_files picks
    (katome_tile_span_for_lengths); 1: tiling does not pay, or KATOME_NO_TILES"""
    h = np.ascontiguousarray(np.asarray(lens), np.uint32)
    return int(_lib.lib().katome_tile_span_for_lengths(k, h.ctypes.data_as(C.POINTER(C.c_uint32)), h.size))


# ---- primitives ------------------------------------------------------------------------------------
def sort_keys(keys, key_bits, key_words, values=None, device=0):
    n = keys.numel() // key_words
    _check(_lib.lib().katome_dev_sort(device, _ptr(keys), _ptr(values), n, key_words, key_bits, _stream()))
    return keys, values


def s2_region_starts(used):
    """where the 256 regions of the ordered count's S2 begin for these used counts when every region is as many whole 4096-key
    tiles as its keys need (257 numbers: the last one is the arrays' length)"""
    u = np.ascontiguousarray(np.asarray(used), np.uint64)
    assert u.size == 256
    start = np.zeros(257, np.uint64)
    _lib.lib().katome_s2_region_starts(u.ctypes.data_as(_lib.u64p), start.ctypes.data_as(_lib.u64p))
    return start


def s2_region_pass(k, used, keys, weights, digits, device=0):
    """keys (int64), weights (int32) and the bytes of their bits 2k - 8 .. 2k - 1 (uint8) laid out in regions at
    s2_region_starts(used) -> the dense (keys, weights) after the one partition pass by those bits (katome_dev_s2_region_pass)"""
    u = np.ascontiguousarray(np.asarray(used), np.uint64)
    n = int(u.sum())
    out_k = torch.empty(max(n, 1), dtype=torch.int64, device=keys.device)
    out_w = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
    _check(_lib.lib().katome_dev_s2_region_pass(device, k, u.ctypes.data_as(_lib.u64p), _ptr(keys), _ptr(weights), _ptr(digits), _ptr(out_k),
                                                _ptr(out_w), _stream()))
    return out_k[:n], out_w[:n]


def count_records(keys, weights, k, rc=False, min_weight=0, n_parts=0, device=0):
    """(key, count) records in any order -- keys int64 [n * nw] on the device, weights int32 [n] or None: every record counts once
    -- counted by sorting as a level of a build is (katome_dev_count_records) -> (keys [m * nw], weights [m], n_out, n_distinct,
    base, count).  Without owners (n_parts = 0) m = n_out and base / count are empty; with them owner p's entries are
    [base[p], base[p] + count[p]) of the m = n returned.  Raises KatomePanic with the count's own status."""
    nw = record_words(k)
    n = keys.numel() // nw
    cap = (2 if rc else 1) * n + 1
    out_k = torch.empty(cap * nw, dtype=torch.int64, device=keys.device)
    out_w = torch.empty(cap, dtype=torch.int32, device=keys.device)
    n_out, n_distinct = C.c_uint64(), C.c_uint64()
    base, count = np.zeros(max(n_parts, 1), np.uint64), np.zeros(max(n_parts, 1), np.uint64)
    _check(_lib.lib().katome_dev_count_records(device, _ptr(keys), _ptr(weights), n, k, int(bool(rc)), min_weight, n_parts, _ptr(out_k), _ptr(out_w), cap,
                                               C.byref(n_out), C.byref(n_distinct), base.ctypes.data_as(_lib.u64p), count.ctypes.data_as(_lib.u64p), _stream()))
    m = n if n_parts else n_out.value
    return out_k[:m * nw], out_w[:m], n_out.value, n_distinct.value, [int(x) for x in base[:n_parts]], [int(x) for x in count[:n_parts]]


def unique_sorted(keys, key_words, device=0):
    n = keys.numel() // key_words
    out = C.c_uint64()
    _check(_lib.lib().katome_dev_unique(device, _ptr(keys), n, key_words, C.byref(out), _stream()))
    return keys.view(-1)[:out.value * key_words]


def replay_edge_removals(pos, mult, n_edges, device=0):
    """remove_paths' swap_removes (pruner.rs:199-217) for marked positions `pos` (ascending, int32/uint32 on the device)
    listed `mult` times each -> (victims in removal order, move_to, move_from, edges left, removals owed to repeats)"""
    u = pos.numel()
    marks = int(mult.to(torch.int64).sum().item()) if u else 0
    victims = torch.empty(max(marks, 1), dtype=torch.int32, device=pos.device)
    to = torch.empty(max(u, 1), dtype=torch.int32, device=pos.device)
    frm = torch.empty(max(u, 1), dtype=torch.int32, device=pos.device)
    counts = (C.c_uint64 * 4)()
    _check(_lib.lib().katome_dev_replay_edge_removals(device, _ptr(pos), _ptr(mult), u, n_edges, _ptr(victims), _ptr(to), _ptr(frm),
                                                      C.cast(counts, C.c_void_p), _stream()))
    m, moves, left, dups = (int(x) for x in counts)
    return victims[:m], to[:moves], frm[:moves], left, dups


def replay_node_removals(die, n_nodes, device=0):
    """remove_single_node after every removed edge (pruner.rs:206-225) for die[t] = (source, target) left without edges by
    edge removal t (-1 = stays) -> (move_to, move_from, nodes left, gave_up)"""
    m = die.numel() // 2
    to = torch.empty(max(2 * m, 1), dtype=torch.int32, device=die.device)
    frm = torch.empty(max(2 * m, 1), dtype=torch.int32, device=die.device)
    counts = (C.c_uint64 * 3)()
    _check(_lib.lib().katome_dev_replay_node_removals(device, _ptr(die), m, n_nodes, _ptr(to), _ptr(frm), C.cast(counts, C.c_void_p), _stream()))
    moves, left, gave_up = (int(x) for x in counts)
    return to[:moves], frm[:moves], left, bool(gave_up)


def replay_edge_removals64(pos, mult, n_edges, device=0):
    """replay_edge_removals on 64-bit positions (int64 tensors; the positions of a graph sharded over several GPUs)"""
    u = pos.numel()
    marks = int(mult.to(torch.int64).sum().item()) if u else 0
    victims = torch.empty(max(marks, 1), dtype=torch.int64, device=pos.device)
    to = torch.empty(max(u, 1), dtype=torch.int64, device=pos.device)
    frm = torch.empty(max(u, 1), dtype=torch.int64, device=pos.device)
    counts = (C.c_uint64 * 4)()
    _check(_lib.lib().katome_dev_replay_edge_removals64(device, _ptr(pos), _ptr(mult), u, n_edges, _ptr(victims), _ptr(to), _ptr(frm),
                                                        C.cast(counts, C.c_void_p), _stream()))
    m, moves, left, dups = (int(x) for x in counts)
    return victims[:m], to[:moves], frm[:moves], left, dups


def replay_node_removals64(die, n_nodes, device=0):
    """replay_node_removals on 64-bit positions (-1 = stays)"""
    m = die.numel() // 2
    to = torch.empty(max(2 * m, 1), dtype=torch.int64, device=die.device)
    frm = torch.empty(max(2 * m, 1), dtype=torch.int64, device=die.device)
    counts = (C.c_uint64 * 3)()
    _check(_lib.lib().katome_dev_replay_node_removals64(device, _ptr(die), m, n_nodes, _ptr(to), _ptr(frm), C.cast(counts, C.c_void_p), _stream()))
    moves, left, gave_up = (int(x) for x in counts)
    return to[:moves], frm[:moves], left, bool(gave_up)


def scan_counts(counts, device=0):
    """exclusive prefix sums (int64, one more entry than counts: the total) of int32/uint32 counts on the device"""
    m = counts.numel()
    offs = torch.empty(m + 1, dtype=torch.int64, device=counts.device)
    _check(_lib.lib().katome_dev_scan_counts(device, _ptr(counts), m, _ptr(offs), _stream()))
    return offs


def rank_in_sorted(sorted_keys, queries, key_bits, key_words, device=0):
    ns, nq = sorted_keys.numel() // key_words, queries.numel() // key_words
    out = torch.empty(max(nq, 1), dtype=torch.int64, device=queries.device)
    _check(_lib.lib().katome_dev_rank(device, _ptr(sorted_keys), ns, key_words, key_bits, _ptr(queries), nq, _ptr(out),
                                      _stream()))
    return out[:nq]


def depth_arrays(k, edge_key, edge_weight, seq, byte_off, lens, encoding="packed", either_strand=False, windows=False, edge_hits=False, flags=None,
                 device=0):
    """katome_dev_depth on the caller's arrays (katome_dev_depth_arrays): edge_key int64 [n_edges * key_words] in any order but
    distinct, edge_weight int32 [n_edges], the query as Builder.depth takes it -> dict of the per-sequence tensors, window_off,
    window_edge / edge_hits (None unless asked for) and the totals.  flags: the raw flag word instead of the three switches"""
    nw = record_words(k)
    ne, n = edge_key.numel() // nw, lens.numel()
    dev = seq.device
    fl = _depth_flags(either_strand, windows, edge_hits) if flags is None else flags
    i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    i32 = lambda m: torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    present, invalid, ssum, mn, mx, woff = i64(n), i64(n), i64(n), i32(n), i32(n), i64(n + 1)
    # (the windows are known only to the call: room for every sequence's len - k + 1)
    cap = int((lens.to(torch.int64) - k + 1).clamp(min=0).sum().item()) if n and (fl & 2) else 0
    wedge = i64(cap) if fl & 2 else None
    hits = i32(ne) if fl & 4 else None
    totals = (C.c_uint64 * 5)()
    _check(_lib.lib().katome_dev_depth_arrays(device, k, _ptr(edge_key), _ptr(edge_weight), ne, DEPTH_ENCODINGS.get(encoding, encoding), fl, _ptr(seq),
                                              seq.numel(), _ptr(byte_off), _ptr(lens), n, _ptr(present), _ptr(invalid), _ptr(ssum), _ptr(mn), _ptr(mx),
                                              _ptr(woff), _ptr(wedge), cap, _ptr(hits), totals, _stream()))
    nwin = int(totals[0])
    return dict(seq_present=present[:n], seq_invalid=invalid[:n], seq_sum=ssum[:n], seq_min=mn[:n], seq_max=mx[:n], seq_window_off=woff[:n + 1],
                window_edge=wedge[:nwin] if wedge is not None else None, edge_hits=hits[:ne] if hits is not None else None, n_seqs=n,
                n_windows=nwin, n_present=int(totals[1]), n_invalid=int(totals[2]), weight_sum=int(totals[3]), n_edges_hit=int(totals[4]), n_edges=ne)


def stats_arrays(edge_src, edge_dst, edge_weight, n_nodes, device=0):
    """CollectionStats of a graph given as device arrays (int64 endpoints below n_nodes -- not checked --, int32/uint32 weights):
    katome_dev_stats_arrays"""
    st = _lib.Stats()
    _check(_lib.lib().katome_dev_stats_arrays(device, _ptr(edge_src), _ptr(edge_dst), _ptr(edge_weight), edge_src.numel(), n_nodes,
                                              C.byref(st), _stream()))
    return collection_stats(st, capacity=(st.node_count, st.edge_count))


def weight_spectrum_arrays(weight, n_bins, device=0):
    """np.uint64[n_bins] histogram of int32/uint32 weights on the device, weights >= n_bins - 1 in the last bin:
    katome_dev_weight_spectrum_arrays"""
    bins = np.zeros(max(int(n_bins), 0), np.uint64)
    _check(_lib.lib().katome_dev_weight_spectrum_arrays(device, _ptr(weight), weight.numel(), bins.ctypes.data_as(_lib.u64p), n_bins,
                                                        _stream()))
    return bins


def release_cache(device=0):
    """hand the library's cached device blocks back to the driver -> bytes the library still holds afterwards (what live
    builders, results and views pin; 0 when everything was closed)"""
    _check(_lib.lib().katome_dev_release_cache(device))
    return cache_stats(device)["held_bytes"]


def cache_stats(device=0):
    out = (C.c_uint64 * 3)()
    _check(_lib.lib().katome_dev_cache_stats(device, out))
    return dict(held_bytes=int(out[0]), free_bytes=int(out[1]), live_blocks=int(out[2]))


def source_ids(edge_keys, k, device=0):
    """distinct source (k-1)-mers of sorted distinct edges, ascending, and each edge's position among them
    -> (node_keys [n_src*nw], edge_src [E])"""
    nw = record_words(k)
    n = edge_keys.numel() // nw
    nodes = torch.empty(max(n, 1) * nw, dtype=torch.int64, device=edge_keys.device)
    src = torch.empty(max(n, 1), dtype=torch.int64, device=edge_keys.device)
    ns = C.c_uint64()
    _check(_lib.lib().katome_dev_source_ids(device, _ptr(edge_keys), n, k, _ptr(nodes), _ptr(src), C.byref(ns), _stream()))
    return nodes[:ns.value * nw], src[:n]


def key_owner(key_words_list, n_parts, core=None):
    """host: owner of one key given as its u64 words (most significant first)"""
    nw = len(key_words_list)
    arr = (C.c_uint64 * nw)(*key_words_list)
    return _lib.lib().katome_key_owner(arr, nw, core[0] if core else 0, core[1] if core else 0, n_parts)


def node_ids(edge_keys, k, device=0):
    """local node numbering of sorted distinct edges -> (node_keys [n_nodes*nw], edge_src [E], edge_dst [E])"""
    nw = record_words(k)
    n = edge_keys.numel() // nw
    nodes = torch.empty(max(2 * n, 1) * nw, dtype=torch.int64, device=edge_keys.device)
    src = torch.empty(max(n, 1), dtype=torch.int64, device=edge_keys.device)
    dst = torch.empty(max(n, 1), dtype=torch.int64, device=edge_keys.device)
    nn = C.c_uint64()
    _check(_lib.lib().katome_dev_node_ids(device, _ptr(edge_keys), n, k, _ptr(nodes), _ptr(src), _ptr(dst), C.byref(nn), _stream()))
    return nodes[:nn.value * nw], src[:n], dst[:n]


def endpoints(edge_keys, k, device=0, want_src=True):
    nw = record_words(k)
    n = edge_keys.numel() // nw
    src, dst = (torch.empty_like(edge_keys) if want_src else None), torch.empty_like(edge_keys)
    _check(_lib.lib().katome_dev_endpoints(device, _ptr(edge_keys), n, k, _ptr(src), _ptr(dst), _stream()))
    return src, dst


def labels(edge_keys, k, device=0):
    nw = record_words(k)
    n = edge_keys.numel() // nw
    stride = 1 + (k + 3) // 4
    out = torch.empty((max(n, 1) * stride + 3) // 4 * 4, dtype=torch.uint8, device=edge_keys.device)
    _check(_lib.lib().katome_dev_labels(device, _ptr(edge_keys), n, k, _ptr(out), _stream()))
    return out[:n * stride].view(n, stride)


def pieces_text(labels, label_off, pieces, k, layout="plain", device=0, first_contig=0):
    """the text kernel on the caller's arrays (katome_dev_pieces_text_numbered; first_contig: contig c's FASTA header reads
    ">katome_<first_contig + c>"): labels uint8 (compress_edge format, label i at
    labels[label_off[i]:label_off[i + 1]], label_off int64 with one more entry than labels), pieces int32/uint32 (label index,
    bit 31 on a piece that begins a contig; None: one whole piece per label) -> (contig_off int64, contig_len int32, text uint8
    of text_bytes rounded up to 16, text_bytes)"""
    tdev = labels.device
    n_labels = label_off.numel() - 1
    n_pieces = pieces.numel() if pieces is not None else n_labels
    nc, nb = C.c_uint64(), C.c_uint64()
    L = _lib.lib()
    _check(L.katome_dev_pieces_text_numbered(device, k, _ptr(labels), _ptr(label_off), n_labels, _ptr(pieces), n_pieces, LAYOUTS[layout],
                                             first_contig, None, None, 0, None, 0, C.byref(nc), C.byref(nb), _stream()))
    cap = (nb.value + 15) // 16 * 16
    off = torch.empty(max(nc.value, 1), dtype=torch.int64, device=tdev)
    length = torch.empty(max(nc.value, 1), dtype=torch.int32, device=tdev)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_pieces_text_numbered(device, k, _ptr(labels), _ptr(label_off), n_labels, _ptr(pieces), n_pieces, LAYOUTS[layout],
                                             first_contig, _ptr(off), _ptr(length), nc.value, _ptr(text), cap, C.byref(nc), C.byref(nb), _stream()))
    return off[:nc.value], length[:nc.value], text, nb.value


def gfa_arrays(k, n_nodes, edge_src, edge_dst, edge_weight, edge_kmers, edge_label_off, edge_label, device=0, label_bytes=None):
    """the GFA kernels on the caller's tensors (katome_dev_gfa_arrays): a graph in the layout of DeviceContigs -- edge_src /
    edge_dst / edge_label_off int64, edge_weight / edge_kmers int32, edge_label uint8 in an allocation that is a multiple of 4
    bytes (label_bytes: how many of them are labels, default all) -> DeviceGfa (text: text_bytes of a buffer rounded up to 16)"""
    tdev = edge_label_off.device
    n_edges = edge_label_off.numel() - 1
    if label_bytes is None:
        label_bytes = edge_label.numel()
    nl, nb = C.c_uint64(), C.c_uint64()
    L = _lib.lib()
    args = (device, k, n_nodes, n_edges, _ptr(edge_src), _ptr(edge_dst), _ptr(edge_weight), _ptr(edge_kmers), _ptr(edge_label_off),
            _ptr(edge_label), label_bytes)
    _check(L.katome_dev_gfa_arrays(*args, None, None, None, 0, C.byref(nl), C.byref(nb), _stream()))
    cap = (nb.value + 15) // 16 * 16
    seg = torch.empty(max(n_edges, 1), dtype=torch.int64, device=tdev)
    first = torch.empty(n_edges + 1, dtype=torch.int64, device=tdev)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_gfa_arrays(*args, _ptr(seg), _ptr(first), _ptr(text), cap, C.byref(nl), C.byref(nb), _stream()))
    return DeviceGfa(n_edges, nl.value, nb.value, text[:nb.value], seg[:n_edges], first)


def gfa_paths_arrays(edge_src, edge_dst, pieces, device=0):
    """the path kernels on the caller's tensors (katome_dev_gfa_paths_arrays): edge_src / edge_dst int64 (the shrunk graph the pieces
    name), pieces int32/uint32 (edge index, bit 31 on a piece that begins a contig) -> (path_text uint8 of text_bytes rounded up to
    16, {n_paths, n_jumps, text_bytes}, path_line_off, path_contig, path_first_piece)"""
    tdev = pieces.device
    counts = (C.c_uint64 * 3)()
    L = _lib.lib()
    args = (device, edge_src.numel(), _ptr(edge_src), _ptr(edge_dst), _ptr(pieces), pieces.numel())
    _check(L.katome_dev_gfa_paths_arrays(*args, None, None, None, 0, None, 0, counts, _stream()))
    n_paths, cap = counts[0], (counts[2] + 15) // 16 * 16
    line_off = torch.empty(n_paths + 1, dtype=torch.int64, device=tdev)
    contig = torch.empty(max(n_paths, 1), dtype=torch.int64, device=tdev)
    first = torch.empty(n_paths + 1, dtype=torch.int64, device=tdev)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_gfa_paths_arrays(*args, _ptr(line_off), _ptr(contig), _ptr(first), n_paths, _ptr(text), cap, counts, _stream()))
    return text, dict(n_paths=counts[0], n_jumps=counts[1], text_bytes=counts[2]), line_off, contig[:n_paths], first


def gfa_strand_paths_arrays(edge_src, edge_dst, edge_twin, pieces, device=0):
    """the path kernels over MERGED segments and the mirror search on the caller's tensors (katome_dev_gfa_strand_paths_arrays):
    gfa_paths_arrays with edge_twin int64 (DeviceGfaStrands.edge_twin: -1 for none) -> (path_text uint8 of text_bytes rounded up to
    16, {n_paths, n_jumps, text_bytes, n_mirrored, n_self_mirror}, path_line_off, path_contig, path_first_piece, path_mirror)"""
    tdev = pieces.device
    counts = (C.c_uint64 * 5)()
    L = _lib.lib()
    args = (device, edge_src.numel(), _ptr(edge_src), _ptr(edge_dst), _ptr(edge_twin), _ptr(pieces), pieces.numel())
    _check(L.katome_dev_gfa_strand_paths_arrays(*args, None, None, None, None, 0, None, 0, counts, _stream()))
    n_paths, cap = counts[0], (counts[2] + 15) // 16 * 16
    line_off = torch.empty(n_paths + 1, dtype=torch.int64, device=tdev)
    contig = torch.empty(max(n_paths, 1), dtype=torch.int64, device=tdev)
    first = torch.empty(n_paths + 1, dtype=torch.int64, device=tdev)
    mirror = torch.empty(max(n_paths, 1), dtype=torch.int64, device=tdev)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_gfa_strand_paths_arrays(*args, _ptr(line_off), _ptr(contig), _ptr(first), _ptr(mirror), n_paths, _ptr(text), cap, counts, _stream()))
    names = ("n_paths", "n_jumps", "text_bytes", "n_mirrored", "n_self_mirror")
    return text, dict(zip(names, counts)), line_off, contig[:n_paths], first, mirror[:n_paths]


def unique_contigs_arrays(labels, label_off, edge_twin, pieces, k, layout="plain", device=0):
    """katome_dev_collapse_unique on the caller's tensors (katome_dev_unique_contigs_arrays): labels / label_off as for pieces_text,
    edge_twin int64 with an entry per label (-1 for none), pieces int32/uint32 -> DeviceUniqueAssembly (text: text_bytes of a
    buffer rounded up to 16, zeros behind them)"""
    tdev = label_off.device
    n_labels = label_off.numel() - 1
    counts = (C.c_uint64 * 5)()
    L = _lib.lib()
    args = (device, k, _ptr(labels), _ptr(label_off), n_labels, _ptr(edge_twin), _ptr(pieces), pieces.numel(), LAYOUTS[layout])
    _check(L.katome_dev_unique_contigs_arrays(*args, None, 0, None, None, None, 0, None, 0, counts, _stream()))
    n, n_kept, cap = counts[0], counts[1], (counts[2] + 15) // 16 * 16
    mirror = torch.empty(max(n, 1), dtype=torch.int64, device=tdev)
    name = torch.empty(max(n_kept, 1), dtype=torch.int64, device=tdev)
    off = torch.empty(max(n_kept, 1), dtype=torch.int64, device=tdev)
    length = torch.empty(max(n_kept, 1), dtype=torch.int32, device=tdev)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_unique_contigs_arrays(*args, _ptr(mirror), n, _ptr(name), _ptr(off), _ptr(length), n_kept, _ptr(text), cap, counts, _stream()))
    return DeviceUniqueAssembly(counts[0], counts[3], counts[4], mirror[:n], counts[1], counts[2], layout, name[:n_kept], off[:n_kept], length[:n_kept], text)


def gfa_coverage_arrays(k, n_nodes, edge_src, edge_dst, edge_weight, edge_kmers, kmer_sum, kmer_min, kmer_max, edge_label_off, edge_label, device=0,
                        label_bytes=None):
    """gfa_arrays with the unitigs' coverage (katome_dev_gfa_coverage_arrays): kmer_sum int64, kmer_min / kmer_max int32 (the
    u64 / u32 bits), one entry per edge -> DeviceGfa whose KC is kmer_sum and whose S lines end in mn / mx"""
    tdev = edge_label_off.device
    n_edges = edge_label_off.numel() - 1
    if label_bytes is None:
        label_bytes = edge_label.numel()
    nl, nb = C.c_uint64(), C.c_uint64()
    L = _lib.lib()
    args = (device, k, n_nodes, n_edges, _ptr(edge_src), _ptr(edge_dst), _ptr(edge_weight), _ptr(edge_kmers), _ptr(kmer_sum), _ptr(kmer_min),
            _ptr(kmer_max), _ptr(edge_label_off), _ptr(edge_label), label_bytes)
    _check(L.katome_dev_gfa_coverage_arrays(*args, None, None, None, 0, C.byref(nl), C.byref(nb), _stream()))
    cap = (nb.value + 15) // 16 * 16
    seg = torch.empty(max(n_edges, 1), dtype=torch.int64, device=tdev)
    first = torch.empty(n_edges + 1, dtype=torch.int64, device=tdev)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_gfa_coverage_arrays(*args, _ptr(seg), _ptr(first), _ptr(text), cap, C.byref(nl), C.byref(nb), _stream()))
    return DeviceGfa(n_edges, nl.value, nb.value, text[:nb.value], seg[:n_edges], first)


def gfa_strands_arrays(k, n_nodes, edge_src, edge_dst, edge_weight, edge_kmers, edge_label_off, edge_label, device=0, label_bytes=None):
    """gfa_arrays with strand twins merged (katome_dev_gfa_strands_arrays) -> DeviceGfaStrands"""
    tdev = edge_label_off.device
    n_edges = edge_label_off.numel() - 1
    if label_bytes is None:
        label_bytes = edge_label.numel()
    counts = (C.c_uint64 * 5)()
    L = _lib.lib()
    args = (device, k, n_nodes, n_edges, _ptr(edge_src), _ptr(edge_dst), _ptr(edge_weight), _ptr(edge_kmers), _ptr(edge_label_off),
            _ptr(edge_label), label_bytes)
    _check(L.katome_dev_gfa_strands_arrays(*args, None, None, None, None, None, 0, counts, _stream()))
    ns, cap = counts[0], (counts[2] + 15) // 16 * 16
    name = torch.empty(max(ns, 1), dtype=torch.int64, device=tdev)
    seg = torch.empty(max(ns, 1), dtype=torch.int64, device=tdev)
    first = torch.empty(ns + 1, dtype=torch.int64, device=tdev)
    twin = torch.empty(max(n_edges, 1), dtype=torch.int64, device=tdev)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_gfa_strands_arrays(*args, _ptr(name), _ptr(seg), _ptr(first), _ptr(twin), _ptr(text), cap, counts, _stream()))
    return DeviceGfaStrands(counts[0], counts[1], counts[2], text[:counts[2]], seg[:ns], first, name[:ns], twin[:n_edges], counts[3], counts[4])


def gfa_part_arrays(k, edge_weight, edge_kmers, edge_label_off, edge_label, first_segment, with_header, link_first, link_b, device=0,
                    label_bytes=None):
    """the numbered GFA writer on the caller's tensors (katome_dev_gfa_part_arrays): one PART of a text whose other parts are
    written elsewhere.  Segment i is named first_segment + i; its links are link_b[link_first[i]:link_first[i + 1]] (int64 tensors;
    link_b holds global numbers as uint64 bit patterns); the header line is written or not -> (text uint8, s_bytes, l_offset,
    l_bytes, segment_off int64): the S part is text[:s_bytes], the L part text[l_offset:l_offset + l_bytes]"""
    tdev = edge_label_off.device
    n_edges = edge_label_off.numel() - 1
    if label_bytes is None:
        label_bytes = edge_label.numel()
    sb, lo, lb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    L = _lib.lib()
    args = (device, k, n_edges, _ptr(edge_weight), _ptr(edge_kmers), _ptr(edge_label_off), _ptr(edge_label), label_bytes, first_segment,
            1 if with_header else 0, _ptr(link_first), _ptr(link_b))
    _check(L.katome_dev_gfa_part_arrays(*args, None, None, 0, C.byref(sb), C.byref(lo), C.byref(lb), _stream()))
    cap = lo.value + (lb.value + 15) // 16 * 16
    seg = torch.empty(max(n_edges, 1), dtype=torch.int64, device=tdev)
    text = torch.full((max(cap, 16),), 0xAA, dtype=torch.uint8, device=tdev)
    _check(L.katome_dev_gfa_part_arrays(*args, _ptr(seg), _ptr(text), cap, C.byref(sb), C.byref(lo), C.byref(lb), _stream()))
    return text[:cap], sb.value, lo.value, lb.value, seg[:n_edges]


def synth_reads(first_read, n_reads, read_len, genome_len, err_rate, n_inject_percent=0, device=0):
    """deterministic synthetic workload, generated in HBM (DESIGN.md 'Synthetic workload')"""
    tdev = torch.device("cuda", device)
    stride = (read_len + 3) // 4
    packed = torch.empty(n_reads * stride + 32, dtype=torch.uint8, device=tdev)
    skip = torch.empty(max(n_reads, 1), dtype=torch.uint8, device=tdev)
    _check(_lib.lib().katome_dev_synth_reads(device, first_read, n_reads, read_len, genome_len, float(err_rate),
                                             n_inject_percent, _ptr(packed), _ptr(skip), _stream()))
    return packed, skip
