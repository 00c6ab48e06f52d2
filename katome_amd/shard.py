"""The sharded (multi-GPU) build from Python: thin bindings of katome_comm_* / katome_dist_* (include/katome_gpu.h).

Everything that moves or computes is in libkatome_gpu.so (katome_amd/csrc/comm.cpp, dist.hip): this module only creates
the communicator of a one-process-per-GPU job -- RCCL, the unique id handed round with torch.distributed; or, for
rehearsals and CPU tests, a transport whose bytes travel through torch.distributed/gloo -- and wraps the handles.
A single-process caller (the Rust shim of INTEGRATION.md) needs none of this: it sets `settings.n_devices`.
"""
import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .build import ContigsStats, KatomePanic, collection_stats, make_settings
from .device import LAYOUTS, Builder, DeviceContigs, _ViewOwner, _ptr, _stream, _view


def _check(status):
    if status != 0:
        raise KatomePanic(status, _lib.last_error())


def shard_range(total_reads, world, rank):
    """contiguous shard of reads for `rank`: (first, count); starts are multiples of 64 reads"""
    first, count = C.c_uint64(), C.c_uint64()
    _lib.lib().katome_shard_range(total_reads, world, rank, C.byref(first), C.byref(count))
    return first.value, count.value


class Comm:
    """one rank's end of the exchange layer"""

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep                      # callbacks must outlive the handle

    @classmethod
    def rccl(cls, rank, world, device, group=None):
        """RCCL over xGMI, one process per GPU: rank 0 makes the unique id, torch.distributed hands it round"""
        L = _lib.lib()
        ident = (C.c_uint8 * 128)()
        if rank == 0:
            _check(L.katome_comm_unique_id(ident))
        if world > 1:
            box = [bytes(ident)]
            dist.broadcast_object_list(box, src=0, group=group)
            ident = (C.c_uint8 * 128)(*box[0])
        h = C.c_void_p()
        _check(L.katome_comm_create_rccl(ident, rank, world, device, C.byref(h)))
        return cls(h)

    @classmethod
    def over_torch(cls, group=None, device=0):
        """the caller's transport: bytes travel through torch.distributed (gloo: staged through the host).  Lets several
        processes share one GPU (RCCL refuses that) and runs the comm layer on CPU-only machines."""
        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def tensor_of(ptr, nbytes, on_device):
            if nbytes == 0:
                return torch.empty(0, dtype=torch.uint8)
            if on_device:
                return _view(ptr, (nbytes,), "|u1", None, torch.device("cuda", device))
            return torch.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=torch.uint8)

        def alltoallv(_user, send, send_off, send_cnt, recv, recv_off, recv_cnt, elem, on_device):
            try:
                s_n = [send_cnt[p] * elem for p in range(world)]
                r_n = [recv_cnt[p] * elem for p in range(world)]
                s_o = [send_off[p] * elem for p in range(world)]
                r_o = [recv_off[p] * elem for p in range(world)]
                s_end, r_end = max(o + n for o, n in zip(s_o, s_n)), max(o + n for o, n in zip(r_o, r_n))
                src = tensor_of(send, s_end, on_device)
                out = tensor_of(recv, r_end, on_device)
                staged = torch.cat([src[o:o + n].cpu() for o, n in zip(s_o, s_n)]) if sum(s_n) else torch.empty(0, dtype=torch.uint8)
                got = torch.empty(sum(r_n), dtype=torch.uint8)
                dist.all_to_all_single(got, staged, output_split_sizes=r_n, input_split_sizes=s_n, group=group)
                at = 0
                for o, n in zip(r_o, r_n):
                    if n:
                        out[o:o + n].copy_(got[at:at + n])
                    at += n
                if on_device:
                    torch.cuda.synchronize()
                return 0
            except Exception as e:     # noqa: BLE001  (nothing may unwind into C)
                print("[katome comm] alltoallv callback failed: %r" % (e,), flush=True)
                return 1

        def allreduce(_user, vals, n, op):
            try:
                t = torch.tensor([vals[i] for i in range(n)], dtype=torch.int64) if n <= 64 else \
                    torch.frombuffer((C.c_int64 * n).from_address(C.addressof(vals.contents)), dtype=torch.int64).clone()
                # u64 values above 2^63 do not occur (counts, histograms, sequence numbers)
                dist.all_reduce(t, op={0: dist.ReduceOp.SUM, 1: dist.ReduceOp.MAX, 2: dist.ReduceOp.MIN}[op], group=group)
                out = t.tolist()
                for i in range(n):
                    vals[i] = out[i]
                return 0
            except Exception as e:     # noqa: BLE001
                print("[katome comm] allreduce callback failed: %r" % (e,), flush=True)
                return 1

        cb = _lib.CommCallbacks(None, _lib.A2A_FN(alltoallv), _lib.ALLREDUCE_FN(allreduce))
        h = C.c_void_p()
        _check(_lib.lib().katome_comm_create_callbacks(C.byref(cb), rank, world, device, C.byref(h)))
        return cls(h, keep=cb)

    @property
    def rank(self):
        return _lib.lib().katome_comm_rank(self._h)

    @property
    def world(self):
        return _lib.lib().katome_comm_world(self._h)

    @property
    def kind(self):
        return _lib.lib().katome_comm_kind(self._h).decode()

    def set_max_message_bytes(self, n):
        _check(_lib.lib().katome_comm_set_max_message_bytes(self._h, n))

    def allreduce(self, values, op="sum"):
        arr = (C.c_uint64 * len(values))(*values)
        _check(_lib.lib().katome_comm_allreduce_u64(self._h, arr, len(values), {"sum": 0, "max": 1, "min": 2}[op]))
        return list(arr)

    def exchange_host(self, send, send_counts, elem_words=1):
        """variable all-to-all of host int64 records (elem_words words each) grouped by destination -> (recv, recv_counts)"""
        send = send.contiguous()
        world = self.world
        sc = (C.c_uint64 * world)(*send_counts)
        rc = (C.c_uint64 * world)()
        cap = 1 << 22
        recv = torch.empty(cap * elem_words, dtype=torch.int64)
        _check(_lib.lib().katome_comm_exchange(self._h, C.c_void_p(send.data_ptr()), sc, C.c_void_p(recv.data_ptr()), cap, rc,
                                               8 * elem_words, 0, None))
        counts = [int(x) for x in rc]
        return recv[:sum(counts) * elem_words], counts

    def close(self):
        if self._h:
            _lib.lib().katome_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RankGraph:
    """this rank's share of the graph (zero-copy views of the builder's device arrays): its edges, disjoint from every
    other rank's, with GLOBAL node ids; the nodes it owns.  By packed key node i has id node_base + i; in the reference's
    numbering edge_id / node_id hold the petgraph index of every edge / node."""

    def __init__(self, g, owner, device):
        ne, nn, nw = g.n_edges, g.n_nodes, g.key_words
        self.n_edges, self.n_nodes, self.total_edges, self.total_nodes = ne, nn, g.total_edges, g.total_nodes
        self.node_base, self.key_words, self.label_stride = g.node_base, nw, g.label_stride
        self.edge_key = _view(g.d_edge_key, (ne, nw), "<i8", owner, device)
        self.edge_weight = _view(g.d_edge_weight, (ne,), "<i4", owner, device)
        self.edge_src = _view(g.d_edge_src, (ne,), "<i8", owner, device)
        self.edge_dst = _view(g.d_edge_dst, (ne,), "<i8", owner, device)
        self.edge_label = _view(g.d_edge_label, (ne, g.label_stride), "|u1", owner, device)
        self.node_key = _view(g.d_node_key, (nn, nw), "<i8", owner, device)
        self.edge_id = _view(g.d_edge_id, (ne,), "<i8", owner, device) if g.d_edge_id else None
        self.node_id = _view(g.d_node_id, (nn,), "<i8", owner, device) if g.d_node_id else None
        # after remove_dead_paths or a stage that may remove edges on the sharded graph: the index each edge had when it was
        # built (petgraph's adjacency order)
        self.edge_age = _view(g.d_edge_age, (ne,), "<i8", owner, device) if g.d_edge_age else None


class RankContigs:
    """this rank's merged edges after ShardedBuilder.shrink() (zero-copy views of the builder's device arrays, valid until
    the next shrink or close): the paths whose head edge this rank holds, with NEW global node ids, and the surviving nodes
    it owns.  head_id: the head edge's global index in the input graph (petgraph index in the reference's numbering, the
    rank's edge base + its local index by packed key).  stats: rank_rounds, cycle_rounds, cycles, longest_path, bytes_sent.
    After shrink(coverage=True) also kmer_sum (int64 view of u64), kmer_min and kmer_max (int32 views of u32) per merged edge
    (None otherwise); the next shrink of either kind drops them."""

    def __init__(self, c, stats, owner, device, cov=None):
        ne, nn, nw = c.n_edges, c.n_nodes, c.key_words
        self.n_edges, self.n_nodes, self.total_edges, self.total_nodes = ne, nn, c.total_edges, c.total_nodes
        self.label_bytes, self.key_words = c.label_bytes, nw
        self.edge_src = _view(c.d_edge_src, (ne,), "<i8", owner, device)
        self.edge_dst = _view(c.d_edge_dst, (ne,), "<i8", owner, device)
        self.edge_weight = _view(c.d_edge_weight, (ne,), "<i4", owner, device)
        self.edge_kmers = _view(c.d_edge_kmers, (ne,), "<i4", owner, device)
        self.edge_label_off = _view(c.d_edge_label_off, (ne + 1,), "<i8", owner, device)
        self.edge_label = _view(c.d_edge_label, (c.label_bytes,), "|u1", owner, device)
        self.edge_head_id = _view(c.d_edge_head_id, (ne,), "<i8", owner, device)
        self.node_id = _view(c.d_node_id, (nn,), "<i8", owner, device)
        self.node_key = _view(c.d_node_key, (nn, nw), "<i8", owner, device)
        self.stats = {f: getattr(stats, f) for f, _ in _lib.DistShrinkStats._fields_}
        self.kmer_sum = self.kmer_min = self.kmer_max = None
        if cov is not None:
            self.kmer_sum = _view(cov.d_kmer_sum, (ne,), "<i8", owner, device)
            self.kmer_min = _view(cov.d_kmer_min, (ne,), "<i4", owner, device)
            self.kmer_max = _view(cov.d_kmer_max, (ne,), "<i4", owner, device)

    sequences = DeviceContigs.sequences


class RankAssembly:
    """this rank's part of the text of the sharded shrink (ShardedBuilder.contigs_text; zero-copy views of the builder's device
    arrays, valid until the next contigs_text or close).  The order is rank-major: contig first_contig + j is this rank's merged
    edge j, text[contig_off[j]:contig_off[j] + contig_len[j]]; the ranks' text[:text_bytes] one after the other, in rank order, are
    the whole text (this rank's part starts at byte text_base of total_text_bytes)."""

    def __init__(self, a, owner, device):
        self._a = a
        self.n_contigs, self.first_contig, self.total_contigs = a.n_contigs, a.first_contig, a.total_contigs
        self.text_bytes, self.text_base, self.total_text_bytes = a.text_bytes, a.text_base, a.total_text_bytes
        self.layout = {v: k for k, v in LAYOUTS.items()}[a.layout]
        self.contig_off = _view(a.d_contig_off, (a.n_contigs,), "<i8", owner, device)
        self.contig_len = _view(a.d_contig_len, (a.n_contigs,), "<i4", owner, device)
        self.text = _view(a.d_text, (a.text_bytes,), "|u1", owner, device)


class RankGfa:
    """this rank's two parts of the GFA 1 text of the sharded shrink (ShardedBuilder.contigs_gfa; zero-copy views of the builder's
    device arrays, valid until the next contigs_gfa or close).  Segments are numbered rank-major like the records of
    contigs_text: segment first_segment + j is this rank's merged edge j.  The whole text is the header line, the ranks' S parts
    in rank order, then their L parts: this rank's s_text (on rank 0 the header line first) starts at byte s_base, its l_text at
    l_base of total_text_bytes.  segment_off[j]: segment j's first base in s_text; the links of segment j are lines
    link_first[j] .. link_first[j + 1] of l_text and link_b holds their second segments' global numbers (uint64 bit patterns)."""

    def __init__(self, g, owner, device):
        self._g = g
        for f in ("n_segments", "first_segment", "total_segments", "n_links", "total_links", "s_bytes", "s_base", "l_bytes", "l_base",
                  "total_text_bytes"):
            setattr(self, f, getattr(g, f))
        self.s_text = _view(g.d_text, (g.s_bytes,), "|u1", owner, device)
        self.l_text = _view(g.d_link_text, (g.l_bytes,), "|u1", owner, device)
        self.segment_off = _view(g.d_segment_off, (g.n_segments,), "<i8", owner, device)
        self.link_first = _view(g.d_link_first, (g.n_segments + 1,), "<i8", owner, device)
        self.link_b = _view(g.d_link_b, (g.n_links,), "<i8", owner, device)


def contig_stats_arrays(comm, kmers, k, genome_len, device=0):
    """Contigs::stats of ALL ranks' contigs from each rank's own k-mer counts (int32 / uint32 device tensor, may be empty; a
    contig's length is its count + k - 1), no rank holding another's (katome_dist_contig_stats_arrays) -> ContigsStats, the same
    on every rank; a tipping point of 0 raises KatomePanic(E_ARG) on every rank.  Collective."""
    st = _lib.ContigStats()
    n = int(kmers.numel())
    _check(_lib.lib().katome_dist_contig_stats_arrays(comm._h, device, _ptr(kmers) if n else None, n, k, int(genome_len), C.byref(st), _stream()))
    return ContigsStats(st.n50, st.l50, st.n90, st.ng50)


class _InnerBuilder(Builder):
    """the single-GPU builder underneath a ShardedBuilder (owned by it): profile counters, and -- on the root after
    gather() -- the stages of device.Builder"""

    def __init__(self, handle, k, rc, device, parent=None):     # noqa: super().__init__ would create a builder
        self.parent = parent                       # the memory behind this builder's views is the parent's to free
        self.k, self.rc, self.device = k, bool(rc), device
        self.nw = _lib.lib().katome_record_words(k)
        self._h = C.c_void_p(handle)
        self.tdev = torch.device("cuda", device)

    def _retain_view(self):
        if self.parent is not None:
            self.parent._retain_view()

    def _release_view(self):
        if self.parent is not None:
            self.parent._release_view()

    def close(self):
        self._h = C.c_void_p()                     # not ours to destroy

    def _destroy(self):
        pass


class ShardedBuilder(_ViewOwner):
    """one rank's share of a sharded build (katome_dist_*); every method is collective"""

    def __init__(self, comm, k, reverse_complement, device=0, table_slots_hint=0, first_seen_order=False):
        self.comm, self.k, self.rc, self.device = comm, k, bool(reverse_complement), device
        self.first_seen = first_seen_order
        s = make_settings(k, reverse_complement=reverse_complement, device=device, table_slots_hint=table_slots_hint,
                          first_seen_order=first_seen_order)
        self._h = C.c_void_p()
        _check(_lib.lib().katome_dist_create(C.byref(s), comm._h, C.byref(self._h)))
        self.tdev = torch.device("cuda", device)

    @property
    def inner(self):
        """the rank's single-GPU builder (a fresh handle wrapper per access: no reference cycle with this object)"""
        return _InnerBuilder(_lib.lib().katome_dist_inner(self._h), self.k, self.rc, self.device, parent=self)

    @property
    def route(self):
        """which records travel: "supermers" / "local" / "tiles" (katome_dist_route)"""
        return _lib.lib().katome_dist_route(self._h).decode()

    def add_reads(self, packed, first_read, n_reads, read_len, skip=None, batch_reads=0):
        _check(_lib.lib().katome_dist_add_reads(self._h, _ptr(packed), first_read, n_reads, read_len, _ptr(skip), batch_reads, _stream()))

    def add_reads_var(self, packed, byte_off, lens, first_window=None, batch_windows=0):
        """this rank's reads of varying length (katome_dist_add_reads_var): `packed` 2-bit bases, read r is lens[r] bases at byte
        byte_off[r] (int64, len(lens) + 1 entries, the last one the bytes in all), device tensors.  first_window: the global
        window of this rank's first read; None (one call per rank, ranks in input order): from every rank's windows with one
        allreduce.  Later calls continue after this rank's earlier ones.  Collective: a rank without reads passes empty tensors."""
        n = int(lens.numel())
        if first_window is None:
            first_window = getattr(self, "_first_window", None)
        if first_window is None:
            mine = int((lens.to(torch.int64) - (self.k - 1)).clamp(min=0).sum().item()) if n else 0
            per_rank = [0] * self.comm.world
            per_rank[self.comm.rank] = mine
            per_rank = self.comm.allreduce(per_rank, "sum")
            first_window = sum(per_rank[:self.comm.rank])
        self._first_window = first_window
        packed_bytes = int(byte_off[n].item()) if n else 0
        _check(_lib.lib().katome_dist_add_reads_var(self._h, _ptr(packed), packed_bytes, _ptr(byte_off), _ptr(lens), n, first_window,
                                                    batch_windows, _stream()))

    def remove_weak_edges(self, threshold):
        _check(_lib.lib().katome_dist_remove_weak_edges(self._h, threshold))

    def finalize(self):
        g = _lib.DistGraph()
        _check(_lib.lib().katome_dist_finalize(self._h, C.byref(g), _stream()))
        return RankGraph(g, self, self.tdev)

    def remove_dead_paths(self):
        """Prunable::remove_dead_paths (pruner.rs:36-82) on the sharded graph, no gather (katome_dist_remove_dead_paths)
        -> (this rank's share of the pruned graph, stats dict)"""
        g, st = _lib.DistGraph(), _lib.PruneStats()
        _check(_lib.lib().katome_dist_remove_dead_paths(self._h, C.byref(g), C.byref(st), _stream()))
        return RankGraph(g, self, self.tdev), {f: getattr(st, f) for f, _ in _lib.PruneStats._fields_}

    # ---- the stages after the first pruning on the sharded graph (katome_dist_*; first-seen order, shares not gathered) ----
    def standardize_contigs(self):
        """Standardizable::standardize_contigs (standardizer.rs:72-122) -> this rank's share.  KATOME_DIST_CONTIGS=table|ranked
        names the route (unset: the replicated table when it fits every rank, list ranking in O(share) memory otherwise)"""
        g = _lib.DistGraph()
        _check(_lib.lib().katome_dist_standardize_contigs(self._h, C.byref(g), _stream()))
        return RankGraph(g, self, self.tdev)

    def standardize_stats(self):
        """what the last standardize_contigs() of this builder did (katome_dist_standardize_stats_read): route (0 table, 1
        ranked), bytes_sent, and on the ranked route rank_rounds, exchanges, contigs, longest_contig, cycle_edges"""
        st = _lib.DistStandardizeStats()
        _check(_lib.lib().katome_dist_standardize_stats_read(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.DistStandardizeStats._fields_}

    def prune_weak_edges(self, threshold):
        """Clean::remove_weak_edges(threshold) (pruner.rs:84-93) at once, in petgraph's numbering -> this rank's share
        (remove_weak_edges is the packed-key threshold applied when the edges are read out)"""
        g = _lib.DistGraph()
        _check(_lib.lib().katome_dist_prune_weak_edges(self._h, threshold, C.byref(g), _stream()))
        return RankGraph(g, self, self.tdev)

    def standardize_edges(self, original_genome_length, threshold):
        """Standardizable::standardize_edges (standardizer.rs:42-70), then prune_weak_edges(1) -> this rank's share"""
        g = _lib.DistGraph()
        _check(_lib.lib().katome_dist_standardize_edges(self._h, original_genome_length, threshold, C.byref(g), _stream()))
        return RankGraph(g, self, self.tdev)

    def shrink(self, coverage=False):
        """Shrinkable::shrink in the traversal-free form (Builder.shrink(mode="fast")) on the sharded graph, no gather
        (katome_dist_shrink) -> RankContigs; the rank's graph stays as it is.  coverage: the result also has kmer_sum, kmer_min
        and kmer_max per merged edge (katome_dist_shrink_coverage)"""
        c, st = _lib.DistContigs(), _lib.DistShrinkStats()
        if coverage:
            cov = _lib.DevCoverage()
            _check(_lib.lib().katome_dist_shrink_coverage(self._h, C.byref(c), C.byref(cov), C.byref(st), _stream()))
            return RankContigs(c, st, self, self.tdev, cov)
        _check(_lib.lib().katome_dist_shrink(self._h, C.byref(c), C.byref(st), _stream()))
        return RankContigs(c, st, self, self.tdev)

    def contigs_text(self, layout="fasta"):
        """the text of the last shrink()'s merged edges on this rank, numbered after the ranks before it
        (katome_dist_contigs_text) -> RankAssembly"""
        a = _lib.DistAssembly()
        _check(_lib.lib().katome_dist_contigs_text(self._h, LAYOUTS[layout], C.byref(a), _stream()))
        return RankAssembly(a, self, self.tdev)

    def contig_stats(self, genome_len):
        """Contigs::stats of all ranks' merged edges after the last shrink(), the same on every rank (katome_dist_contig_stats)"""
        st = _lib.ContigStats()
        _check(_lib.lib().katome_dist_contig_stats(self._h, int(genome_len), C.byref(st), _stream()))
        return ContigsStats(st.n50, st.l50, st.n90, st.ng50)

    def save_contigs(self, assembly, path):
        """the file of the last contigs_text(), every rank writing its part at its offset (katome_dist_contigs_save)"""
        import os
        _check(_lib.lib().katome_dist_contigs_save(self._h, C.byref(assembly._a), os.fsencode(path)))

    def contigs_gfa(self, coverage=False):
        """the unitig graph of the last shrink() as GFA 1, no gather: the links joined across ranks, this rank's S and L parts
        written on the device (katome_dist_contigs_gfa) -> RankGfa.  coverage: KC is the sum of each unitig's k-mer counts and the
        S lines end in mn / mx (katome_dist_contigs_gfa_coverage; needs shrink(coverage=True)).  Collective"""
        g = _lib.DistGfa()
        entry = _lib.lib().katome_dist_contigs_gfa_coverage if coverage else _lib.lib().katome_dist_contigs_gfa
        _check(entry(self._h, C.byref(g), _stream()))
        return RankGfa(g, self, self.tdev)

    def save_gfa(self, gfa, path):
        """the file of the last contigs_gfa(), every rank writing its two parts at their offsets (katome_dist_gfa_save)"""
        import os
        _check(_lib.lib().katome_dist_gfa_save(self._h, C.byref(gfa._g), os.fsencode(path)))

    def stats(self):
        """CollectionStats of the WHOLE graph as it stands, the same on every rank, no gather (katome_dist_graph_stats).
        May re-order this rank's node arrays (the links are rebuilt where a stage dropped them): take graph() again afterwards"""
        st = _lib.Stats()
        _check(_lib.lib().katome_dist_graph_stats(self._h, C.byref(st), _stream()))
        return collection_stats(st, capacity=(st.node_count, st.edge_count))

    def weight_spectrum(self, n_bins):
        """np.uint64[n_bins] weight spectrum of the WHOLE graph on every rank (katome_dist_weight_spectrum)"""
        bins = np.zeros(max(int(n_bins), 0), np.uint64)
        _check(_lib.lib().katome_dist_weight_spectrum(self._h, bins.ctypes.data_as(_lib.u64p), n_bins, _stream()))
        return bins

    def graph(self):
        """this rank's share as it stands (katome_dist_current_graph)"""
        g = _lib.DistGraph()
        _check(_lib.lib().katome_dist_current_graph(self._h, C.byref(g)))
        return RankGraph(g, self, self.tdev)

    def gather(self, root=0):
        """FIRST_SEEN_ORDER: the whole graph to `root` in the reference's index order -> on the root a builder on which
        remove_dead_paths / remove_weak_edges / standardize_* / shrink / graph() work (None elsewhere)"""
        h = C.c_void_p()
        _check(_lib.lib().katome_dist_gather(self._h, root, C.byref(h), _stream()))
        return _InnerBuilder(h.value, self.k, self.rc, self.device, parent=self) if h.value else None

    def exchange_stats(self):
        """{phase: dict(calls, bytes_out, max_message_bytes, ms)} since the last read"""
        L = _lib.lib()
        n = L.katome_dist_exchange_count()
        out = (C.c_uint64 * (4 * n))()
        _check(L.katome_dist_exchange_read(self._h, out))
        return {L.katome_dist_exchange_name(i).decode(): dict(calls=out[4 * i], bytes_out=out[4 * i + 1],
                                                             max_message_bytes=out[4 * i + 2], ms=out[4 * i + 3] / 1000.0)
                for i in range(n) if out[4 * i]}

    def _destroy(self):
        if self._h:
            _lib.lib().katome_dist_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass


class DistBuild:
    """bench.py's N > 1 job: the synthetic workload sharded over the ranks, resident in HBM before the timed region"""

    def __init__(self, wl, comm, batch_reads=0, timer=None, first_seen_order=False, min_weight=0, table_factor=2.2,
                 prune=False):
        from . import device as kd
        self.wl, self.comm, self.batch_reads, self.timer = wl, comm, batch_reads, timer
        self.first_seen, self.min_weight, self.table_factor, self.prune = first_seen_order, min_weight, table_factor, prune
        self.dev = torch.cuda.current_device()
        self.first, self.n_local = shard_range(wl.reads, comm.world, comm.rank)
        self.packed, skip = kd.synth_reads(self.first, self.n_local, wl.read_len, wl.genome_len, wl.err_rate,
                                           wl.n_inject_percent, device=self.dev)
        self.skip = skip if wl.n_inject_percent else None
        local_ok = self.n_local - (int(skip[:self.n_local].sum().item()) if wl.n_inject_percent else 0)
        self.accepted_total = comm.allreduce([local_ok], "sum")[0]
        self.exchange = {}

    def build(self):
        wl = self.wl
        hint = int(wl.expected_distinct_canonical() * self.table_factor) if self.table_factor else 0
        b = ShardedBuilder(self.comm, wl.k, wl.reverse_complement, self.dev, table_slots_hint=hint, first_seen_order=self.first_seen)
        try:
            b.inner.profile(self.timer is not None)
            if self.min_weight:
                b.remove_weak_edges(self.min_weight)
            b.add_reads(self.packed, self.first, self.n_local, wl.read_len, self.skip, self.batch_reads)
            self.route = b.route
            g = b.finalize()
            n_edges, n_nodes = g.total_edges, g.total_nodes
            if self.prune:                                  # BASELINE config 5: the pruner pass, on the sharded graph
                pg, _ = b.remove_dead_paths()
                n_edges, n_nodes = pg.total_edges, pg.total_nodes
            if self.timer is not None:
                self.timer.add(b.inner.profile_read())
                for name, x in b.exchange_stats().items():
                    acc = self.exchange.setdefault(name, dict(calls=0, bytes_out=0, max_message_bytes=0, ms=0.0))
                    acc["calls"] += x["calls"]; acc["bytes_out"] += x["bytes_out"]; acc["ms"] += x["ms"]
                    acc["max_message_bytes"] = max(acc["max_message_bytes"], x["max_message_bytes"])
            return n_edges, n_nodes
        finally:
            b.close()
