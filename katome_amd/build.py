"""Host-side mirror of the reference's build interface for the GPU path.

Mirrors (names, argument meaning, error behaviour):
  * `Config<P>` and `InputFileType`          -- reference src/katome/config.rs:5-37
  * `set_global_k_sizes`                     -- prelude.rs:34-43
  * `Build::create(input_files, ft, reverse_complement, minimal_weight_threshold) -> (Self, usize)`
                                             -- algorithms/builder.rs:42-54
  * `Stats<CollectionStats>::stats`          -- stats/collections.rs:38-89,137-168
The reference panics on every failure (builder.rs:62,67,71,148,153; pt_graph.rs:278); here a
non-zero status of the C ABI is re-raised as `KatomePanic` carrying the same message, which is
what the Rust shim of INTEGRATION.md does with `panic!`.
"""
import ctypes as C
import enum
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib

# prelude.rs:21-25 -- the reference keeps k in `static mut` globals
K_SIZE = 40
K1_SIZE = 39
COMPRESSED_K1_SIZE = 10


class KatomePanic(RuntimeError):
    """A failure the reference reports by panicking."""

    def __init__(self, status, message):
        super().__init__("%s: %s" % (_lib.STATUS.get(status, status), message))
        self.status = status
        self.name = _lib.STATUS.get(status, str(status))
        self.message = message


def _check(status):
    if status != 0:
        raise KatomePanic(status, _lib.last_error())


def set_global_k_sizes(k_size: int):
    """prelude.rs:34-43"""
    global K_SIZE, K1_SIZE, COMPRESSED_K1_SIZE
    assert k_size > 1
    K_SIZE = k_size
    K1_SIZE = k_size - 1
    COMPRESSED_K1_SIZE = (K1_SIZE + 3) // 4


class InputFileType(enum.IntEnum):
    """config.rs:5-14; parsing is case-insensitive like utils.rs:15-19"""
    Fasta = 0
    Fastq = 1
    BFCounter = 2

    @classmethod
    def parse(cls, text: str) -> "InputFileType":
        for m in cls:
            if m.name.lower() == text.lower():
                return m
        raise ValueError("Bad value %r for InputFileType" % text)


@dataclass
class Config:
    """config.rs:18-37"""
    input_files: List[str]
    input_file_type: InputFileType
    output_file: str = ""
    original_genome_length: int = 0
    minimal_weight_threshold: int = 0
    k_mer_size: int = 40
    reverse_complement: bool = True


def _round2(x):
    # stats/collections.rs:84-89 (f64::round = half away from zero; values here are >= 0)
    return None if x is None else float(np.floor(x * 100.0 + 0.5) / 100.0)


@dataclass
class CollectionStats:
    """stats/collections.rs:38-57; equality ignores capacity and rounds the averages to 2 dp (71-82)"""
    node_count: int = 0
    edge_count: int = 0
    max_edge_weight: Optional[int] = None
    avg_edge_weight: Optional[float] = None
    max_in_degree: Optional[int] = None
    max_out_degree: Optional[int] = None
    avg_out_degree: Optional[float] = None
    incoming_vert_count: Optional[int] = None
    outgoing_vert_count: Optional[int] = None
    capacity: tuple = field(default=(0, None), compare=False)

    def __eq__(self, other):
        return (self.node_count == other.node_count and self.edge_count == other.edge_count and
                self.max_edge_weight == other.max_edge_weight and
                _round2(self.avg_edge_weight) == _round2(other.avg_edge_weight) and
                self.max_in_degree == other.max_in_degree and self.max_out_degree == other.max_out_degree and
                _round2(self.avg_out_degree) == _round2(other.avg_out_degree) and
                self.incoming_vert_count == other.incoming_vert_count and
                self.outgoing_vert_count == other.outgoing_vert_count)

    @classmethod
    def with_counts(cls, node_count, edge_count):
        return cls(node_count=node_count, edge_count=edge_count)


def collection_stats(st, capacity=(0, None)) -> CollectionStats:
    """a katome_stats (_lib.Stats) as the reference's CollectionStats"""
    return CollectionStats(
        node_count=st.node_count, edge_count=st.edge_count, max_edge_weight=st.max_edge_weight,
        avg_edge_weight=st.avg_edge_weight, max_in_degree=st.max_in_degree, max_out_degree=st.max_out_degree,
        avg_out_degree=st.avg_out_degree, incoming_vert_count=st.incoming_vert_count,
        outgoing_vert_count=st.outgoing_vert_count, capacity=capacity)


class ContigsStats:
    """stats/contigs.rs:11-23"""

    def __init__(self, n50=0, l50=0, n90=0, ng50=0):
        self.n50, self.l50, self.n90, self.ng50 = n50, l50, n90, ng50

    def astuple(self):
        return (self.n50, self.l50, self.n90, self.ng50)

    def __eq__(self, other):
        return self.astuple() == (other.astuple() if isinstance(other, ContigsStats) else tuple(other))

    def __repr__(self):
        return "ContigsStats(n50=%d, l50=%d, n90=%d, ng50=%d)" % self.astuple()


def contig_stats(lengths, genome_length) -> ContigsStats:
    """Contigs::stats (stats/contigs.rs:31-89) from the contigs' lengths (katome_contig_stats_of: host, pure); a tipping point of
    0 with contigs present, where the reference panics, raises KatomePanic(E_ARG)"""
    a = np.ascontiguousarray(lengths, dtype=np.uint64)
    st = _lib.ContigStats()
    _check(_lib.lib().katome_contig_stats_of(a.ctypes.data_as(_lib.u64p), len(a), int(genome_length), C.byref(st)))
    return ContigsStats(st.n50, st.l50, st.n90, st.ng50)


class _COwned:
    """a result the C library owns: its pointer and the names of the symbols that free it and write its text.  Keeps the C
    result until it is collected."""
    _free = None
    _save = None

    def __init__(self, ptr):
        self._ptr = ptr

    def save_to_file(self, path):
        """the result's text as a file (katome_*_save; for an Assembly: Contigs::save_to_file, asm/mod.rs:57-72): a path that
        cannot be created raises KatomePanic(E_OPEN)"""
        _check(getattr(_lib.lib(), self._save)(self._ptr, os.fsencode(path)))

    def __del__(self):
        try:
            getattr(_lib.lib(), self._free)(self._ptr)
        except Exception:       # interpreter shutdown
            pass


def _array(ptr, n, dtype=np.uint64):
    """a copy of the n elements at ptr (n = 0: the pointer is not read)"""
    return np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dtype)


def _text(ptr, n):
    return bytes(np.ctypeslib.as_array(ptr, (n,))) if n else b""


class Assembly(_COwned):
    """result of GpuGraph.assemble: the contigs (list of str, in the reference's order), the FASTA text Contigs::save_to_file
    writes, Contigs::stats, number_of_read_bytes and the collapse walk's counters.  Keeps the C result until it is collected."""
    _free, _save = "katome_assembly_free", "katome_assembly_save"

    def __init__(self, ap):
        super().__init__(ap)
        a = ap.contents
        nc = a.n_contigs
        self.k, self.read_bytes, self.n_contigs = a.k, a.read_bytes, nc
        self.fasta = _text(a.text, a.text_bytes)
        off, length = _array(a.contig_off, nc).tolist(), _array(a.contig_len, nc).tolist()
        self.contigs = [self.fasta[o:o + n].decode() for o, n in zip(off, length)]
        self.stats = ContigsStats(a.stats.n50, a.stats.l50, a.stats.n90, a.stats.ng50)
        self.collapse_stats = {f: getattr(a.collapse, f) for f, _ in _lib.CollapseStats._fields_}


class Gfa(_COwned):
    """result of GpuGraph.gfa: the unitig graph as GFA 1 (include/katome_gpu.h has the format).  text: the file's bytes;
    segment_off[i]: offset of segment i's first base; link_first[a] .. link_first[a + 1]: the L lines of segment a.  Keeps the C
    result until it is collected."""
    _free, _save = "katome_gfa_free", "katome_gfa_save"

    def __init__(self, gp):
        super().__init__(gp)
        self._gp = gp
        g = gp.contents
        ns, nb = g.n_segments, g.text_bytes
        self.k, self.read_bytes, self.n_segments, self.n_links, self.text_bytes = g.k, g.read_bytes, ns, g.n_links, nb
        self.text = _text(g.text, nb + getattr(g, "path_bytes", 0))      # (with paths: their lines follow, and `text` is the whole file)
        self.segment_off = _array(g.segment_off, ns)
        self.link_first = _array(g.link_first, ns + 1)

    def _strands(self, g):
        """the fields of the merged form"""
        self.n_edges, self.n_unpaired, self.n_self_twins = g.n_edges, g.n_unpaired, g.n_self_twins
        self.segment_name = _array(g.segment_name, g.n_segments)
        self.edge_twin = _array(g.edge_twin, g.n_edges)


class GfaStrands(Gfa):
    """result of GpuGraph.gfa(merge_strands=True): the same with strand twins merged into one segment and +/- links.  S line s is
    merged edge segment_name[s]; edge_twin[i]: the merged edge that is edge i's reverse complement (2^64 - 1: none); n_edges merged
    edges, n_unpaired of them without a twin, n_self_twins their own"""
    _free, _save = "katome_gfa_strands_free", "katome_gfa_strands_save"

    def __init__(self, gp):
        super().__init__(gp)
        self._strands(gp.contents)


class GfaPaths(Gfa):
    """the GFA half of GpuGraph.assemble_gfa: the collapse's shrunk graph as H, S and L lines (text[:text_bytes], segment_off,
    link_first as in Gfa) and its contigs as P lines (path_text = text[text_bytes:], path_bytes of them): path j is the line at
    path_line_off[j] of path_text, a run of contig path_contig[j] whose first piece is piece path_first_piece[j]; n_jumps = n_paths
    - n_contigs.  `text` is the whole file"""
    _free, _save = "katome_gfa_paths_free", "katome_gfa_paths_save"

    def __init__(self, gp):
        super().__init__(gp)
        g = gp.contents
        npaths = g.n_paths
        self.n_paths, self.n_jumps, self.path_bytes = npaths, g.n_jumps, g.path_bytes
        self.path_text = self.text[g.text_bytes:]
        self.path_line_off = _array(g.path_line_off, npaths + 1)
        self.path_contig = _array(g.path_contig, npaths)
        self.path_first_piece = _array(g.path_first_piece, npaths + 1)


class GfaStrandPaths(GfaPaths):
    """the GFA half of GpuGraph.assemble_gfa(merge_strands=True): the collapse's shrunk graph with strand twins merged (the fields
    of GfaStrands) and its contigs as P lines over the merged segments (the fields of GfaPaths; a piece reads <rep><o>).
    path_mirror[j]: the smallest path that spells the same molecule from its other end (2^64 - 1: none); n_mirrored paths have
    one, n_self_mirror are their own"""
    _free, _save = "katome_gfa_strand_paths_free", "katome_gfa_strand_paths_save"

    def __init__(self, gp):
        super().__init__(gp)
        g = gp.contents
        self._strands(g)
        self.n_mirrored, self.n_self_mirror = g.n_mirrored, g.n_self_mirror
        self.path_mirror = _array(g.path_mirror, g.n_paths)

    def unique_paths(self):
        """the indices j with no mirror or mirror(j) >= j: one path per molecule"""
        return [j for j, q in enumerate(self.path_mirror.tolist()) if q == 2 ** 64 - 1 or q >= j]


class UniqueAssembly(_COwned):
    """the strand-unique half of GpuGraph.assemble_unique (include/katome_gpu.h, katome_dev_collapse_unique, has the definitions):
    contigs -- the kept ones, one strand per molecule with all its copies, as strings --, names -- their numbers in the full
    assembly, ascending --, contig_mirror[c] -- the smallest contig that spells c's molecule from its other end by pieces (2^64 - 1:
    none; n_mirrored have one, n_self_mirror are their own) --, stats -- Contigs::stats of the kept contigs -- and fasta, the kept
    records of the full FASTA byte for byte.  Keeps the C result until it is collected."""
    _free, _save = "katome_unique_assembly_free", "katome_unique_assembly_save"

    def __init__(self, up):
        super().__init__(up)
        u = up.contents
        nk = u.n_kept
        self.k, self.read_bytes, self.n_contigs, self.n_kept = u.k, u.read_bytes, u.n_contigs, nk
        self.n_mirrored, self.n_self_mirror = u.n_mirrored, u.n_self_mirror
        self.fasta = _text(u.text, u.text_bytes)
        self.contig_mirror = _array(u.contig_mirror, u.n_contigs)
        self.names = _array(u.kept_name, nk).tolist()
        off, length = _array(u.kept_off, nk).tolist(), _array(u.kept_len, nk).tolist()
        self.contigs = [self.fasta[o:o + n].decode() for o, n in zip(off, length)]
        self.stats = ContigsStats(u.stats.n50, u.stats.l50, u.stats.n90, u.stats.ng50)


def _assemble_gfa_result(rc, ap, gp, cls=GfaPaths):
    """-> (Assembly, GfaPaths); a path that could not be created: both were made all the same, and travel with the exception (`.result`)"""
    result = (Assembly(ap) if ap else None, cls(gp) if gp else None)
    if rc != 0:
        err = KatomePanic(rc, _lib.last_error())
        err.result = result
        raise err
    return result


class Depth(_COwned):
    """result of GpuGraph.depth (katome_depth_paths; include/katome_gpu.h has the definitions): per query record, in file order,
    seq_present, seq_invalid, seq_sum (uint64) and seq_min, seq_max (uint32; nothing present: all ones and 0); the totals; edge_hits
    (uint32 per edge of the graph) when asked for, else None.  Keeps the C result until it is collected."""
    _free = "katome_depth_free"

    def __init__(self, dp):
        super().__init__(dp)
        d = dp.contents
        for f in ("read_bytes", "n_records", "n_windows", "n_present", "n_invalid", "n_edges", "n_edges_hit", "weight_sum"):
            setattr(self, f, int(getattr(d, f)))
        n = self.n_records
        self.seq_present, self.seq_invalid, self.seq_sum = _array(d.seq_present, n), _array(d.seq_invalid, n), _array(d.seq_sum, n)
        self.seq_min, self.seq_max = _array(d.seq_min, n, np.uint32), _array(d.seq_max, n, np.uint32)
        self.edge_hits = (_array(d.edge_hits, self.n_edges, np.uint32) if d.edge_hits else None)


def _gfa_result(rc, gp, cls=Gfa):
    """a path that could not be created: the GFA was made all the same, and travels with the exception (`.result`)"""
    if rc != 0:
        err = KatomePanic(rc, _lib.last_error())
        err.result = cls(gp) if gp else None
        raise err
    return cls(gp)


FLAG_FIRST_SEEN_ORDER = 1
FLAG_REMOVE_DEAD_PATHS = 2
FLAG_RANKS_SHARE_DEVICE = 4
FLAG_PATH_COVERAGE = 8


def make_settings(k, file_type=InputFileType.Fastq, reverse_complement=False, min_weight=0, device=0,
                  table_slots_hint=0, first_seen_order=False, remove_dead_paths=False, n_devices=1,
                  ranks_share_device=False, path_coverage=False):
    """n_devices: GPUs of this node to build on (device .. device+n-1; one rank per GPU inside the call);
    ranks_share_device: all those ranks on `device` -- the rehearsal of the sharded route on a one-GPU box;
    path_coverage: GpuUnitigs.gfa*'s KC is the sum of the unitig's k-mer counts, with mn / mx tags (KATOME_FLAG_PATH_COVERAGE)"""
    s = _lib.Settings()
    s.k = k
    s.file_type = int(file_type)
    s.reverse_complement = 1 if reverse_complement else 0
    s.flags = ((FLAG_FIRST_SEEN_ORDER if first_seen_order else 0) | (FLAG_REMOVE_DEAD_PATHS if remove_dead_paths else 0) |
               (FLAG_RANKS_SHARE_DEVICE if ranks_share_device else 0) | (FLAG_PATH_COVERAGE if path_coverage else 0))
    s.min_weight = min_weight
    s.device = device
    s.table_slots_hint = table_slots_hint
    s.n_devices = n_devices
    return s


def _paths(paths):
    return (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])


def _enc(path):
    return os.fsencode(path) if path is not None else None


class _Reads:
    """where a host entry's reads come from: every entry of the C ABI exists as katome_<entry>_files and katome_<entry>_packed,
    which differ in the arguments between the settings and the entry's own.  Holds the arrays those arguments point into."""

    def __init__(self, twin, *args, keep=None):
        self.twin, self.args, self._keep = twin, args, keep

    @classmethod
    def files(cls, input_files):
        return cls("files", _paths(input_files), len(input_files))

    @classmethod
    def packed(cls, packed, n_reads, read_len, skip):
        """2-bit packed reads (numpy uint8) and, optionally, one byte per read: not 0 = leave the read out"""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
        return cls("packed", packed.ctypes.data, n_reads, read_len, None if skip is None else skip.ctypes.data, keep=(packed, skip))

    def call(self, symbol, settings, *tail):
        """katome_<symbol with this source's word in it>(settings, the reads, *tail) -> status"""
        return getattr(_lib.lib(), symbol.format(self.twin))(C.byref(settings), *self.args, *tail)


class GpuGraph:
    """The collection the GPU build produces: what `Convert<GpuGIR> for PtGraph` consumes.

    Arrays (numpy views of the C result, which lives as long as any of them does): edge_src/edge_dst (dense node ids),
    edge_weight (u32), edge_label ([n_edges, 1+ceil(k/4)] compress_edge format), edge_key / node_key (packed k-mers /
    (k-1)-mers, [n, key_words] u64, most significant word first).
    """

    class _Owner(_COwned):
        """frees the katome_graph when the last array that views it is gone"""
        _free = "katome_graph_free"

    def __init__(self, gptr):
        g = gptr.contents
        owner = GpuGraph._Owner(gptr)
        ne, nn, nw = g.n_edges, g.n_nodes, g.key_words
        self.k = g.k
        self.n_nodes, self.n_edges, self.read_bytes = nn, ne, g.read_bytes
        self.key_words, self.label_stride = nw, g.label_stride

        def arr(ptr, shape, dtype):
            n = int(np.prod(shape))
            if n == 0:
                return np.zeros(shape, dtype)
            buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(C.addressof(ptr.contents))
            buf._owner = owner                      # numpy keeps `buf` as the arrays' base, `buf` keeps the C result
            return np.frombuffer(buf, dtype=dtype).reshape(shape)

        self.edge_src = arr(g.edge_src, (ne,), np.uint64)
        self.edge_dst = arr(g.edge_dst, (ne,), np.uint64)
        self.edge_weight = arr(g.edge_weight, (ne,), np.uint32)
        self.edge_label = arr(g.edge_label, (ne, g.label_stride), np.uint8)
        self.edge_key = arr(g.edge_key, (ne, nw), np.uint64)
        self.node_key = arr(g.node_key, (nn, nw), np.uint64)
        # first-seen index each edge had before remove_dead_paths / remove_weak_edges re-numbered it (None: age == index)
        self.edge_age = arr(g.edge_age, (ne,), np.uint32) if bool(g.edge_age) else None
        self._gptr, self._owner, self._stats = gptr, owner, None      # (stats: on the first stats() call, as in the reference)

    # ---- Build::create (builder.rs:42-54) ----------------------------------------------------
    @classmethod
    def _create(cls, reads, s, stages, original_genome_length, stage_stats):
        gp = C.POINTER(_lib.Graph)()
        described = None
        if stage_stats:
            described = (_lib.Stats * (len(stages or "") + 1))()
            _check(reads.call("katome_build_{}_staged_stats", s, (stages or "").encode(), original_genome_length, described, C.byref(gp)))
        elif stages:
            _check(reads.call("katome_build_{}_staged", s, stages.encode(), original_genome_length, C.byref(gp)))
        else:
            _check(reads.call("katome_build_{}", s, C.byref(gp)))
        g = cls(gp)                                   # the arrays view the C result and free it with their last reference
        if described is not None:
            g.stage_stats = [collection_stats(st) for st in described]
        return g, g.read_bytes

    @classmethod
    def create(cls, input_files, ft, reverse_complement, minimal_weight_threshold=0, device=0, first_seen_order=False,
               remove_dead_paths=False, stages=None, original_genome_length=0, n_devices=1, ranks_share_device=False,
               stage_stats=False):
        """-> (GpuGraph, number_of_read_bytes); uses the global k set by set_global_k_sizes.
        stage_stats: also describe the graph on the device where assemble_with_graph logs it (graph.log_stats(),
        asm/basic_assembler.rs:58-75): g.stage_stats is a list of CollectionStats, entry 0 the graph as built (after the
        pruning remove_dead_paths asks for), entry i the graph after the i-th letter of `stages`.
        stages: stages of assemble_with_graph to run on the device after the build, e.g. "dcwced" = everything before
        collapse (d remove_dead_paths, c standardize_contigs, w remove_weak_edges(minimal_weight_threshold),
        e standardize_edges(original_genome_length, k, minimal_weight_threshold)); needs first_seen_order.
        first_seen_order: number edges and nodes as the reference's petgraph does (order of first insertion).
        remove_dead_paths: also run Prunable::remove_dead_paths (pruner.rs:36-82) as assemble() does next
        (asm/basic_assembler.rs:58-62); needs first_seen_order."""
        s = make_settings(K_SIZE, ft, reverse_complement, minimal_weight_threshold, device,
                          first_seen_order=first_seen_order, remove_dead_paths=remove_dead_paths, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return cls._create(_Reads.files(input_files), s, stages, original_genome_length, stage_stats)

    @classmethod
    def create_from_packed(cls, packed, n_reads, read_len, skip=None, reverse_complement=False, device=0, k=None,
                           first_seen_order=False, remove_dead_paths=False, n_devices=1, ranks_share_device=False,
                           table_slots_hint=0, stages=None, original_genome_length=0, minimal_weight_threshold=0,
                           stage_stats=False):
        """Same build from 2-bit packed reads (numpy uint8), the synthetic-workload entry.  stages / original_genome_length /
        minimal_weight_threshold / stage_stats: as for create(); with n_devices > 1 the stages run on the sharded graph when
        KATOME_DIST_STAGES=sharded is set or the graph is too big to gather, else on the gathered one."""
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, minimal_weight_threshold, device,
                          table_slots_hint=table_slots_hint, first_seen_order=first_seen_order,
                          remove_dead_paths=remove_dead_paths, n_devices=n_devices, ranks_share_device=ranks_share_device)
        return cls._create(_Reads.packed(packed, n_reads, read_len, skip), s, stages, original_genome_length, stage_stats)

    # ---- BasicAsm::assemble (asm/basic_assembler.rs:17-27,58-80) ----------------------------------
    @staticmethod
    def _assemble(reads, s, original_genome_length, output_file):
        ap = C.POINTER(_lib.Assembly)()
        rc = reads.call("katome_assemble_{}", s, original_genome_length, _enc(output_file), C.byref(ap))
        if rc != 0:
            if ap:                      # (a path that could not be created: the assembly was made all the same)
                _lib.lib().katome_assembly_free(ap)
            _check(rc)
        return Assembly(ap)

    @staticmethod
    def assemble(input_files, ft, reverse_complement, minimal_weight_threshold, original_genome_length, output_file=None, device=0,
                 n_devices=1, ranks_share_device=False):
        """the build in the reference's numbering, the stages "dcwced", collapse, Contigs::stats and -- with output_file --
        Contigs::save_to_file, all behind one call (katome_assemble_files) -> Assembly; uses the global k"""
        s = make_settings(K_SIZE, ft, reverse_complement, minimal_weight_threshold, device, first_seen_order=True, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return GpuGraph._assemble(_Reads.files(input_files), s, original_genome_length, output_file)

    @staticmethod
    def assemble_from_packed(packed, n_reads, read_len, skip=None, reverse_complement=False, minimal_weight_threshold=0,
                             original_genome_length=0, output_file=None, device=0, k=None, n_devices=1, ranks_share_device=False):
        """the same from 2-bit packed reads (numpy uint8; katome_assemble_packed)"""
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, minimal_weight_threshold, device,
                          first_seen_order=True, n_devices=n_devices, ranks_share_device=ranks_share_device)
        return GpuGraph._assemble(_Reads.packed(packed, n_reads, read_len, skip), s, original_genome_length, output_file)

    # ---- the assembly and a second form of it from the same collapse, each with a file of its own ---------
    @staticmethod
    def _assemble_with(reads, s, entry, struct, cls, original_genome_length, fasta_file, second_file):
        ap, gp = C.POINTER(_lib.Assembly)(), C.POINTER(struct)()
        rc = reads.call(entry, s, original_genome_length, _enc(fasta_file), _enc(second_file), C.byref(ap), C.byref(gp))
        return _assemble_gfa_result(rc, ap, gp, cls)

    _WITH_GFA = {False: ("katome_assemble_gfa_{}", _lib.GfaPaths, GfaPaths),
                 True: ("katome_assemble_gfa_strands_{}", _lib.GfaStrandPaths, GfaStrandPaths)}
    _WITH_UNIQUE = ("katome_assemble_unique_{}", _lib.UniqueAssembly, UniqueAssembly)

    # the contigs as P lines over the unitigs
    @staticmethod
    def assemble_gfa(input_files, ft, reverse_complement, minimal_weight_threshold, original_genome_length, fasta_file=None, gfa_file=None,
                     device=0, n_devices=1, ranks_share_device=False, merge_strands=False):
        """assemble() and, from the same collapse, the GFA of its shrunk graph with every contig as P lines over the segments (one
        line per run of properly linked pieces; katome_assemble_gfa_files) -> (Assembly, GfaPaths); fasta_file / gfa_file: the
        two files; uses the global k.  merge_strands: strand twins as one segment, +/- in links and paths, and every path's mirror
        (katome_assemble_gfa_strands_files) -> (Assembly, GfaStrandPaths)"""
        s = make_settings(K_SIZE, ft, reverse_complement, minimal_weight_threshold, device, first_seen_order=True, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return GpuGraph._assemble_with(_Reads.files(input_files), s, *GpuGraph._WITH_GFA[bool(merge_strands)], original_genome_length,
                                       fasta_file, gfa_file)

    @staticmethod
    def assemble_gfa_from_packed(packed, n_reads, read_len, skip=None, reverse_complement=False, minimal_weight_threshold=0,
                                 original_genome_length=0, fasta_file=None, gfa_file=None, device=0, k=None, n_devices=1,
                                 ranks_share_device=False, merge_strands=False):
        """the same from 2-bit packed reads (numpy uint8; katome_assemble_gfa_packed, katome_assemble_gfa_strands_packed)"""
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, minimal_weight_threshold, device,
                          first_seen_order=True, n_devices=n_devices, ranks_share_device=ranks_share_device)
        return GpuGraph._assemble_with(_Reads.packed(packed, n_reads, read_len, skip), s, *GpuGraph._WITH_GFA[bool(merge_strands)],
                                       original_genome_length, fasta_file, gfa_file)

    # the strand-unique form: one FASTA record per molecule
    @staticmethod
    def assemble_unique(input_files, ft, reverse_complement, minimal_weight_threshold, original_genome_length, fasta_file=None, unique_file=None,
                        device=0, n_devices=1, ranks_share_device=False):
        """assemble() and, from the same collapse, its strand-unique form: of every molecule's two strands the one whose first copy
        comes first, with all its copies, under the contigs' original numbers (katome_assemble_unique_files) -> (Assembly,
        UniqueAssembly); fasta_file: all contigs, unique_file: the kept ones; uses the global k"""
        s = make_settings(K_SIZE, ft, reverse_complement, minimal_weight_threshold, device, first_seen_order=True, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return GpuGraph._assemble_with(_Reads.files(input_files), s, *GpuGraph._WITH_UNIQUE, original_genome_length, fasta_file, unique_file)

    @staticmethod
    def assemble_unique_from_packed(packed, n_reads, read_len, skip=None, reverse_complement=False, minimal_weight_threshold=0,
                                    original_genome_length=0, fasta_file=None, unique_file=None, device=0, k=None, n_devices=1,
                                    ranks_share_device=False):
        """the same from 2-bit packed reads (numpy uint8; katome_assemble_unique_packed)"""
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, minimal_weight_threshold, device,
                          first_seen_order=True, n_devices=n_devices, ranks_share_device=ranks_share_device)
        return GpuGraph._assemble_with(_Reads.packed(packed, n_reads, read_len, skip), s, *GpuGraph._WITH_UNIQUE, original_genome_length,
                                       fasta_file, unique_file)

    # ---- depth of query files against the graph ----------------------------------------------------
    @staticmethod
    def depth(input_files, ft, reverse_complement, query_files, query_ft, k=None, stages="", threshold=0, original_genome_length=0, device=0,
              n_devices=1, first_seen_order=None, ranks_share_device=False, either_strand=False, edge_hits=False):
        """the build from the read files as create() runs it (stage letters as there; they need the reference's numbering), then every
        record of the query files (FASTA or FASTQ) looked up in the graph, in file order (katome_depth_paths) -> Depth.
        first_seen_order: None = whenever stage letters or several devices ask for it.  k: None = the global k"""
        fso = bool(stages) or n_devices > 1 if first_seen_order is None else first_seen_order
        s = make_settings(K_SIZE if k is None else k, ft, reverse_complement, threshold, device, first_seen_order=fso, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        dp = C.POINTER(_lib.Depth)()
        _check(_lib.lib().katome_depth_paths(C.byref(s), _paths(input_files), len(input_files), (stages or "").encode(), original_genome_length,
                                             _paths(query_files), len(query_files), int(query_ft), (1 if either_strand else 0) | (4 if edge_hits else 0),
                                             C.byref(dp)))
        return Depth(dp)

    # ---- the unitig graph as GFA 1 ---------------------------------------------------------------
    @staticmethod
    def _gfa(reads, s, stages, original_genome_length, output_file, merge_strands):
        entry, struct, cls = (("katome_gfa_strands_{}", _lib.GfaStrands, GfaStrands) if merge_strands else
                              ("katome_gfa_{}", _lib.Gfa, Gfa))
        gp = C.POINTER(struct)()
        rc = reads.call(entry, s, (stages or "").encode(), original_genome_length, _enc(output_file), C.byref(gp))
        return _gfa_result(rc, gp, cls)

    @staticmethod
    def gfa(input_files, ft, reverse_complement, threshold, stages="", original_genome_length=0, output_file=None, device=0, n_devices=1,
            first_seen_order=None, ranks_share_device=False, merge_strands=False):
        """the build, the stage letters (as for create(); they need the reference's numbering), shrink and the GFA of the unitig
        graph -- with output_file also the file --, all behind one call (katome_gfa_files) -> Gfa; uses the global k.
        first_seen_order: None = whenever stage letters or several devices ask for it (an empty `stages` on one device builds by
        packed key and shrinks in the fast form).  merge_strands: strand twins as one segment with +/- links
        (katome_gfa_strands_files) -> GfaStrands"""
        if first_seen_order is None:
            first_seen_order = bool(stages) or n_devices > 1
        s = make_settings(K_SIZE, ft, reverse_complement, threshold, device, first_seen_order=first_seen_order, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return GpuGraph._gfa(_Reads.files(input_files), s, stages, original_genome_length, output_file, merge_strands)

    @staticmethod
    def gfa_from_packed(packed, n_reads, read_len, skip=None, reverse_complement=False, threshold=0, stages="", original_genome_length=0,
                        output_file=None, device=0, k=None, n_devices=1, first_seen_order=None, ranks_share_device=False, merge_strands=False):
        """the same from 2-bit packed reads (numpy uint8; katome_gfa_packed, katome_gfa_strands_packed)"""
        if first_seen_order is None:
            first_seen_order = bool(stages) or n_devices > 1
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, threshold, device,
                          first_seen_order=first_seen_order, n_devices=n_devices, ranks_share_device=ranks_share_device)
        return GpuGraph._gfa(_Reads.packed(packed, n_reads, read_len, skip), s, stages, original_genome_length, output_file, merge_strands)

    # ---- Stats<CollectionStats> (stats/collections.rs:137-168) ---------------------------------
    def stats(self) -> CollectionStats:
        # a pass over the host arrays (degrees, weights): Stats::stats is its own call in the reference too, not part of create
        if self._stats is None:
            st = _lib.Stats()
            _check(_lib.lib().katome_graph_stats(self._gptr, C.byref(st)))
            self._stats = collection_stats(st, capacity=(self.n_nodes, self.n_edges))
        return self._stats

    # ---- helpers for parity checks --------------------------------------------------------------
    def key_ints(self, which="edge"):
        """packed keys as Python ints"""
        a = self.edge_key if which == "edge" else self.node_key
        if self.key_words == 1:
            return [int(x) for x in a[:, 0]]
        return [(int(h) << 64) | int(l) for h, l in a]

    def kmer_strings(self):
        k = self.k
        return [_int_to_kmer(v, k) for v in self.key_ints("edge")]

    def multiset(self):
        """sorted list of (k-mer string, weight) -- the parity observable"""
        return sorted(zip(self.kmer_strings(), (int(w) for w in self.edge_weight)))


class GpuContigs:
    """The build followed by Shrinkable::shrink (shrinker.rs:165-209): one edge per maximal straight path.

    edge_seq: the paths as ACGT strings (decoded from the compress_edge labels); edge_weight: weight of each path's
    first k-mer; edge_kmers: k-mers merged into each edge; edge_src/edge_dst: ids into node_key."""

    def __init__(self, cptr):
        c = cptr.contents
        ne, nn, nw = c.n_edges, c.n_nodes, c.key_words
        self.k, self.n_nodes, self.n_edges, self.read_bytes, self.key_words = c.k, nn, ne, c.read_bytes, nw
        self.edge_src, self.edge_dst = _array(c.edge_src, ne), _array(c.edge_dst, ne)
        self.edge_weight, self.edge_kmers = _array(c.edge_weight, ne, np.uint32), _array(c.edge_kmers, ne, np.uint32)
        self.edge_label_off = _array(c.edge_label_off, ne + 1)
        self.edge_label = _array(c.edge_label, c.label_bytes, np.uint8)
        self.node_key = _array(c.node_key, nn * nw).reshape(nn, nw)
        self.edge_seq = []
        for i in range(ne):
            b = self.edge_label[int(self.edge_label_off[i]):int(self.edge_label_off[i + 1])]
            bases = "".join("ACGT"[(int(x) >> sh) & 3] for x in b[1:] for sh in (6, 4, 2, 0))
            self.edge_seq.append(bases[:len(bases) - int(b[0])])

    @classmethod
    def _create(cls, reads, s):
        cp = C.POINTER(_lib.Contigs)()
        _check(reads.call("katome_shrink_{}", s, C.byref(cp)))
        try:
            c = cls(cp)
        finally:
            _lib.lib().katome_contigs_free(cp)
        return c, c.read_bytes

    @classmethod
    def create(cls, input_files, ft, reverse_complement, minimal_weight_threshold=0, device=0, first_seen_order=False,
               remove_dead_paths=False, n_devices=1, ranks_share_device=False):
        """Build::create, optionally remove_dead_paths, then shrink -- the start of assemble_with_graph
        (asm/basic_assembler.rs:58-65) -> (GpuContigs, number_of_read_bytes)"""
        s = make_settings(K_SIZE, ft, reverse_complement, minimal_weight_threshold, device,
                          first_seen_order=first_seen_order, remove_dead_paths=remove_dead_paths, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return cls._create(_Reads.files(input_files), s)

    @classmethod
    def create_from_packed(cls, packed, n_reads, read_len, skip=None, reverse_complement=False, device=0, k=None,
                           first_seen_order=False, remove_dead_paths=False, n_devices=1, ranks_share_device=False):
        """The same from 2-bit packed reads (numpy uint8; katome_shrink_packed).  With n_devices > 1 the shrink runs on the
        graph gathered to one GPU, or with KATOME_DIST_SHRINK=sharded in the traversal-free form on the sharded graph."""
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, 0, device,
                          first_seen_order=first_seen_order, remove_dead_paths=remove_dead_paths, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return cls._create(_Reads.packed(packed, n_reads, read_len, skip), s)

    def contigs(self):
        """sorted (sequence, weight): the parity observable"""
        return sorted(zip(self.edge_seq, (int(w) for w in self.edge_weight)))


class UnitigsGfa:
    """what GpuUnitigs.gfa / gfa_from_packed hand back (katome_unitigs_gfa): n_segments, n_links, text_bytes (of the GFA text),
    total_bases, longest, read_bytes, k, n_devices and, over several GPUs, shrink (the sharded shrink's counters)"""

    def __init__(self, u):
        for f in ("n_segments", "n_links", "text_bytes", "total_bases", "longest", "read_bytes", "k", "n_devices"):
            setattr(self, f, getattr(u, f))
        self.shrink = {f: getattr(u.shrink, f) for f, _ in _lib.DistShrinkStats._fields_}


class GpuUnitigs:
    """The build, the stages asked for and the traversal-free shrink, ending in the unitigs' FASTA file and Contigs::stats
    (katome_unitigs_*): n_contigs, text_bytes (of the FASTA text), total_bases, longest, read_bytes, k, n_devices, stats
    (ContigsStats) and, over several GPUs, shrink (the sharded shrink's counters).  With n_devices > 1 everything runs on the
    ranks' shares, never a gather; the file's records are then in rank-major order."""

    def __init__(self, u):
        for f in ("n_contigs", "text_bytes", "total_bases", "longest", "read_bytes", "k", "n_devices"):
            setattr(self, f, getattr(u, f))
        self.stats = ContigsStats(u.stats.n50, u.stats.l50, u.stats.n90, u.stats.ng50)
        self.shrink = {f: getattr(u.shrink, f) for f, _ in _lib.DistShrinkStats._fields_}

    @staticmethod
    def _run(reads, s, entry, struct, cls, stages, original_genome_length, output_file):
        """a katome_unitigs*_ entry: the caller's plain struct filled in -> (cls of it, number_of_read_bytes)"""
        u = struct()
        _check(reads.call(entry, s, (stages or "").encode(), original_genome_length, _enc(output_file), C.byref(u)))
        return cls(u), u.read_bytes

    @staticmethod
    def gfa(input_files, ft, reverse_complement, minimal_weight_threshold=0, output_file=None, stages=None, original_genome_length=0,
            device=0, first_seen_order=False, remove_dead_paths=False, n_devices=1, ranks_share_device=False, coverage=False):
        """the same pipeline ending in the unitig GRAPH as a GFA 1 file (katome_unitigs_gfa_files): with n_devices > 1 the links are
        joined across the ranks' shares, never a gather, and segment <i> is the record >katome_<i> of create()'s file ->
        (UnitigsGfa, number_of_read_bytes); uses the global k.  coverage: KC is the sum of each unitig's k-mer counts and the S
        lines end in mn / mx (KATOME_FLAG_PATH_COVERAGE)"""
        s = make_settings(K_SIZE, ft, reverse_complement, minimal_weight_threshold, device, first_seen_order=first_seen_order,
                          remove_dead_paths=remove_dead_paths, n_devices=n_devices, ranks_share_device=ranks_share_device,
                          path_coverage=coverage)
        return GpuUnitigs._run(_Reads.files(input_files), s, "katome_unitigs_gfa_{}", _lib.UnitigsGfa, UnitigsGfa, stages,
                               original_genome_length, output_file)

    @staticmethod
    def gfa_from_packed(packed, n_reads, read_len, skip=None, reverse_complement=False, minimal_weight_threshold=0, output_file=None,
                        stages=None, original_genome_length=0, device=0, k=None, first_seen_order=False, remove_dead_paths=False,
                        n_devices=1, ranks_share_device=False, coverage=False):
        """the same from 2-bit packed reads (numpy uint8; katome_unitigs_gfa_packed)"""
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, minimal_weight_threshold, device,
                          first_seen_order=first_seen_order, remove_dead_paths=remove_dead_paths, n_devices=n_devices,
                          ranks_share_device=ranks_share_device, path_coverage=coverage)
        return GpuUnitigs._run(_Reads.packed(packed, n_reads, read_len, skip), s, "katome_unitigs_gfa_{}", _lib.UnitigsGfa, UnitigsGfa,
                               stages, original_genome_length, output_file)

    @classmethod
    def create(cls, input_files, ft, reverse_complement, minimal_weight_threshold=0, output_file=None, stages=None,
               original_genome_length=0, device=0, first_seen_order=False, remove_dead_paths=False, n_devices=1,
               ranks_share_device=False):
        """-> (GpuUnitigs, number_of_read_bytes); uses the global k.  stages / remove_dead_paths need first_seen_order"""
        s = make_settings(K_SIZE, ft, reverse_complement, minimal_weight_threshold, device, first_seen_order=first_seen_order,
                          remove_dead_paths=remove_dead_paths, n_devices=n_devices, ranks_share_device=ranks_share_device)
        return cls._run(_Reads.files(input_files), s, "katome_unitigs_{}", _lib.Unitigs, cls, stages, original_genome_length, output_file)

    @classmethod
    def create_from_packed(cls, packed, n_reads, read_len, skip=None, reverse_complement=False, minimal_weight_threshold=0,
                           output_file=None, stages=None, original_genome_length=0, device=0, k=None, first_seen_order=False,
                           remove_dead_paths=False, n_devices=1, ranks_share_device=False):
        """the same from 2-bit packed reads (numpy uint8; katome_unitigs_packed)"""
        s = make_settings(K_SIZE if k is None else k, InputFileType.Fastq, reverse_complement, minimal_weight_threshold, device,
                          first_seen_order=first_seen_order, remove_dead_paths=remove_dead_paths, n_devices=n_devices,
                          ranks_share_device=ranks_share_device)
        return cls._run(_Reads.packed(packed, n_reads, read_len, skip), s, "katome_unitigs_{}", _lib.Unitigs, cls, stages,
                        original_genome_length, output_file)


def _int_to_kmer(v, k):
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def ingest_files(input_files, ft, k):
    """Host ingest alone (check_files + record scan + ACGT filter + 2-bit packing): builder.rs:57-77,118-165"""
    s = make_settings(k, ft)
    rp = C.POINTER(_lib.Reads)()
    _check(_lib.lib().katome_ingest_files(C.byref(s), _paths(input_files), len(input_files), C.byref(rp)))
    r = rp.contents
    try:
        out = dict(n_records=r.n_records, n_reads=r.n_reads, read_bytes=r.read_bytes, packed_bytes=r.packed_bytes,
                   total_windows=r.total_windows, fixed_len=r.fixed_len,
                   packed=(np.ctypeslib.as_array(r.packed, (max(r.packed_bytes, 1),)).copy()[:r.packed_bytes]),
                   byte_off=np.ctypeslib.as_array(r.byte_off, (r.n_reads + 1,)).copy(),
                   len=(np.ctypeslib.as_array(r.len, (max(r.n_reads, 1),)).copy()[:r.n_reads]))
    finally:
        _lib.lib().katome_reads_free(rp)
    return out
