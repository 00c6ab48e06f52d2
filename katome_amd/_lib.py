"""ctypes binding of include/katome_gpu.h (the same symbols a Rust `extern "C"` block binds)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)

STATUS = {0: "OK", -1: "E_PATH", -2: "E_IS_DIR", -3: "E_NOT_EXIST", -4: "E_OPEN", -5: "E_PARSE", -6: "E_SHORT_READ",
          -7: "E_ARG", -8: "E_DEVICE", -9: "E_OOM", -10: "E_UNSUPPORTED"}


class Settings(C.Structure):
    _fields_ = [("k", C.c_uint32), ("file_type", C.c_uint8), ("reverse_complement", C.c_uint8), ("flags", C.c_uint16),
                ("min_weight", C.c_uint32), ("device", C.c_int32), ("table_slots_hint", C.c_uint64),
                ("n_devices", C.c_int32), ("_reserved", C.c_uint32)]


class Graph(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_edges", C.c_uint64), ("read_bytes", C.c_uint64), ("k", C.c_uint32),
                ("key_words", C.c_uint32), ("label_stride", C.c_uint32), ("_pad", C.c_uint32),
                ("edge_src", u64p), ("edge_dst", u64p), ("edge_weight", u32p), ("edge_label", u8p),
                ("edge_key", u64p), ("node_key", u64p), ("edge_age", u32p)]


class Stats(C.Structure):
    _fields_ = [("node_count", C.c_uint64), ("edge_count", C.c_uint64), ("max_edge_weight", C.c_uint32),
                ("_pad", C.c_uint32), ("avg_edge_weight", C.c_double), ("max_in_degree", C.c_uint64),
                ("max_out_degree", C.c_uint64), ("avg_out_degree", C.c_double), ("incoming_vert_count", C.c_uint64),
                ("outgoing_vert_count", C.c_uint64)]


class Reads(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_reads", C.c_uint64), ("read_bytes", C.c_uint64),
                ("packed_bytes", C.c_uint64), ("total_windows", C.c_uint64), ("fixed_len", C.c_uint32),
                ("_pad", C.c_uint32), ("packed", u8p), ("byte_off", u64p), ("len", u32p)]


class PruneStats(C.Structure):
    _fields_ = [("passes", C.c_uint64), ("walks", C.c_uint64), ("dead_walks", C.c_uint64), ("marked", C.c_uint64),
                ("removed_edges", C.c_uint64), ("removed_by_duplicates", C.c_uint64), ("removed_nodes", C.c_uint64),
                ("host_ms", C.c_double), ("total_ms", C.c_double)]


class Contigs(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_edges", C.c_uint64), ("label_bytes", C.c_uint64), ("read_bytes", C.c_uint64),
                ("k", C.c_uint32), ("key_words", C.c_uint32), ("edge_src", u64p), ("edge_dst", u64p), ("edge_weight", u32p),
                ("edge_kmers", u32p), ("edge_label_off", u64p), ("edge_label", u8p), ("node_key", u64p)]


class DevContigs(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_edges", C.c_uint64), ("label_bytes", C.c_uint64), ("key_words", C.c_uint32),
                ("_pad", C.c_uint32), ("d_edge_src", C.c_void_p), ("d_edge_dst", C.c_void_p), ("d_edge_weight", C.c_void_p),
                ("d_edge_kmers", C.c_void_p), ("d_edge_label_off", C.c_void_p), ("d_edge_label", C.c_void_p),
                ("d_node_key", C.c_void_p)]


class DevCoverage(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("d_kmer_sum", C.c_void_p), ("d_kmer_min", C.c_void_p), ("d_kmer_max", C.c_void_p)]


class Depth(C.Structure):
    """katome_depth"""
    _fields_ = [("read_bytes", C.c_uint64), ("n_records", C.c_uint64), ("n_windows", C.c_uint64), ("n_present", C.c_uint64), ("n_invalid", C.c_uint64),
                ("n_edges", C.c_uint64), ("n_edges_hit", C.c_uint64), ("weight_sum", C.c_uint64), ("seq_present", u64p), ("seq_invalid", u64p),
                ("seq_sum", u64p), ("seq_min", C.POINTER(C.c_uint32)), ("seq_max", C.POINTER(C.c_uint32)), ("edge_hits", C.POINTER(C.c_uint32))]


class DevDepth(C.Structure):
    """katome_dev_depth_result"""
    _fields_ = [("n_seqs", C.c_uint64), ("n_windows", C.c_uint64), ("n_present", C.c_uint64), ("n_invalid", C.c_uint64), ("n_edges", C.c_uint64),
                ("n_edges_hit", C.c_uint64), ("weight_sum", C.c_uint64), ("d_seq_present", C.c_void_p), ("d_seq_invalid", C.c_void_p),
                ("d_seq_sum", C.c_void_p), ("d_seq_min", C.c_void_p), ("d_seq_max", C.c_void_p), ("d_seq_window_off", C.c_void_p),
                ("d_window_edge", C.c_void_p), ("d_edge_hits", C.c_void_p)]


class DevAssembly(C.Structure):
    _fields_ = [("n_contigs", C.c_uint64), ("text_bytes", C.c_uint64), ("layout", C.c_uint32), ("_pad", C.c_uint32),
                ("d_contig_off", C.c_void_p), ("d_contig_len", C.c_void_p), ("d_text", C.c_void_p)]


class CollapseStats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_pieces", "n_contigs", "nodes_left", "edges_left", "steps", "ambiguity_cuts", "self_loops",
                                          "simple_loops", "scc_restarts", "nodes_removed", "ambiguity_moves", "shrunk_nodes",
                                          "shrunk_edges")] + [("shrink_host_ms", C.c_double), ("host_ms", C.c_double),
                                                              ("text_ms", C.c_double)]


class ContigStats(C.Structure):
    _fields_ = [("n50", C.c_uint64), ("l50", C.c_uint64), ("n90", C.c_uint64), ("ng50", C.c_uint64)]


class Assembly(C.Structure):
    _fields_ = [("n_contigs", C.c_uint64), ("text_bytes", C.c_uint64), ("read_bytes", C.c_uint64), ("k", C.c_uint32),
                ("layout", C.c_uint32), ("contig_off", u64p), ("contig_len", u32p), ("text", u8p), ("stats", ContigStats),
                ("collapse", CollapseStats)]


class DevGfa(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("d_text", C.c_void_p),
                ("d_segment_off", C.c_void_p), ("d_link_first", C.c_void_p)]


class Gfa(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("read_bytes", C.c_uint64),
                ("k", C.c_uint32), ("_pad", C.c_uint32), ("text", u8p), ("segment_off", u64p), ("link_first", u64p)]


class DevGfaStrands(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("n_unpaired", C.c_uint64),
                ("n_self_twins", C.c_uint64), ("d_text", C.c_void_p), ("d_segment_name", C.c_void_p), ("d_segment_off", C.c_void_p),
                ("d_link_first", C.c_void_p), ("d_edge_twin", C.c_void_p)]


class GfaStrands(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("read_bytes", C.c_uint64),
                ("k", C.c_uint32), ("_pad", C.c_uint32), ("text", u8p), ("segment_off", u64p), ("link_first", u64p),
                ("n_edges", C.c_uint64), ("n_unpaired", C.c_uint64), ("n_self_twins", C.c_uint64), ("segment_name", u64p),
                ("edge_twin", u64p)]


class DevGfaPaths(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("d_text", C.c_void_p),
                ("d_segment_off", C.c_void_p), ("d_link_first", C.c_void_p), ("n_paths", C.c_uint64), ("n_jumps", C.c_uint64),
                ("path_bytes", C.c_uint64), ("d_path_text", C.c_void_p), ("d_path_line_off", C.c_void_p), ("d_path_contig", C.c_void_p),
                ("d_path_first_piece", C.c_void_p)]


class GfaPaths(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("read_bytes", C.c_uint64),
                ("k", C.c_uint32), ("_pad", C.c_uint32), ("text", u8p), ("segment_off", u64p), ("link_first", u64p),
                ("n_paths", C.c_uint64), ("n_jumps", C.c_uint64), ("path_bytes", C.c_uint64), ("path_line_off", u64p),
                ("path_contig", u64p), ("path_first_piece", u64p)]


class DevGfaStrandPaths(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("n_unpaired", C.c_uint64),
                ("n_self_twins", C.c_uint64), ("d_text", C.c_void_p), ("d_segment_name", C.c_void_p), ("d_segment_off", C.c_void_p),
                ("d_link_first", C.c_void_p), ("d_edge_twin", C.c_void_p), ("n_paths", C.c_uint64), ("n_jumps", C.c_uint64),
                ("path_bytes", C.c_uint64), ("d_path_text", C.c_void_p), ("d_path_line_off", C.c_void_p), ("d_path_contig", C.c_void_p),
                ("d_path_first_piece", C.c_void_p), ("n_mirrored", C.c_uint64), ("n_self_mirror", C.c_uint64), ("d_path_mirror", C.c_void_p),
                ("n_edges", C.c_uint64)]


class DevUniqueAssembly(C.Structure):
    _fields_ = [("n_contigs", C.c_uint64), ("n_mirrored", C.c_uint64), ("n_self_mirror", C.c_uint64), ("d_contig_mirror", C.c_void_p),
                ("n_kept", C.c_uint64), ("text_bytes", C.c_uint64), ("layout", C.c_uint32), ("_pad", C.c_uint32),
                ("d_kept_name", C.c_void_p), ("d_kept_off", C.c_void_p), ("d_kept_len", C.c_void_p), ("d_text", C.c_void_p)]


class UniqueAssembly(C.Structure):
    _fields_ = [("n_contigs", C.c_uint64), ("n_kept", C.c_uint64), ("text_bytes", C.c_uint64), ("read_bytes", C.c_uint64),
                ("k", C.c_uint32), ("_pad", C.c_uint32), ("n_mirrored", C.c_uint64), ("n_self_mirror", C.c_uint64),
                ("contig_mirror", u64p), ("kept_name", u64p), ("kept_off", u64p), ("kept_len", C.POINTER(C.c_uint32)), ("text", u8p),
                ("stats", ContigStats)]


class GfaStrandPaths(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("read_bytes", C.c_uint64),
                ("k", C.c_uint32), ("_pad", C.c_uint32), ("text", u8p), ("segment_off", u64p), ("link_first", u64p),
                ("n_edges", C.c_uint64), ("n_unpaired", C.c_uint64), ("n_self_twins", C.c_uint64), ("segment_name", u64p),
                ("edge_twin", u64p), ("n_paths", C.c_uint64), ("n_jumps", C.c_uint64), ("path_bytes", C.c_uint64), ("path_line_off", u64p),
                ("path_contig", u64p), ("path_first_piece", u64p), ("n_mirrored", C.c_uint64), ("n_self_mirror", C.c_uint64),
                ("path_mirror", u64p)]


class DevGraph(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_edges", C.c_uint64), ("key_words", C.c_uint32),
                ("label_stride", C.c_uint32), ("d_edge_key", C.c_void_p), ("d_edge_weight", C.c_void_p),
                ("d_edge_src", C.c_void_p), ("d_edge_dst", C.c_void_p), ("d_edge_label", C.c_void_p),
                ("d_node_key", C.c_void_p), ("d_edge_age", C.c_void_p)]


class DistGraph(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("n_nodes", C.c_uint64), ("total_edges", C.c_uint64), ("total_nodes", C.c_uint64),
                ("node_base", C.c_uint64), ("key_words", C.c_uint32), ("label_stride", C.c_uint32),
                ("d_edge_key", C.c_void_p), ("d_edge_weight", C.c_void_p), ("d_edge_src", C.c_void_p),
                ("d_edge_dst", C.c_void_p), ("d_edge_label", C.c_void_p), ("d_node_key", C.c_void_p),
                ("d_edge_id", C.c_void_p), ("d_node_id", C.c_void_p), ("d_edge_age", C.c_void_p)]


class DistContigs(C.Structure):
    _fields_ = [("n_edges", C.c_uint64), ("n_nodes", C.c_uint64), ("total_edges", C.c_uint64), ("total_nodes", C.c_uint64),
                ("label_bytes", C.c_uint64), ("key_words", C.c_uint32), ("_pad", C.c_uint32),
                ("d_edge_src", C.c_void_p), ("d_edge_dst", C.c_void_p), ("d_edge_weight", C.c_void_p), ("d_edge_kmers", C.c_void_p),
                ("d_edge_label_off", C.c_void_p), ("d_edge_label", C.c_void_p), ("d_edge_head_id", C.c_void_p),
                ("d_node_id", C.c_void_p), ("d_node_key", C.c_void_p)]


class DistShrinkStats(C.Structure):
    _fields_ = [("rank_rounds", C.c_uint32), ("cycle_rounds", C.c_uint32), ("cycles", C.c_uint64), ("longest_path", C.c_uint64),
                ("bytes_sent", C.c_uint64)]


class DistAssembly(C.Structure):
    _fields_ = [("n_contigs", C.c_uint64), ("first_contig", C.c_uint64), ("total_contigs", C.c_uint64), ("text_bytes", C.c_uint64),
                ("text_base", C.c_uint64), ("total_text_bytes", C.c_uint64), ("layout", C.c_uint32), ("_pad", C.c_uint32),
                ("d_contig_off", C.c_void_p), ("d_contig_len", C.c_void_p), ("d_text", C.c_void_p)]


class Unitigs(C.Structure):
    _fields_ = [("n_contigs", C.c_uint64), ("text_bytes", C.c_uint64), ("total_bases", C.c_uint64), ("longest", C.c_uint64),
                ("read_bytes", C.c_uint64), ("k", C.c_uint32), ("n_devices", C.c_uint32), ("stats", ContigStats),
                ("shrink", DistShrinkStats)]


class DistGfa(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("first_segment", C.c_uint64), ("total_segments", C.c_uint64), ("n_links", C.c_uint64),
                ("total_links", C.c_uint64), ("s_bytes", C.c_uint64), ("s_base", C.c_uint64), ("l_bytes", C.c_uint64),
                ("l_base", C.c_uint64), ("total_text_bytes", C.c_uint64), ("d_text", C.c_void_p), ("d_link_text", C.c_void_p),
                ("d_segment_off", C.c_void_p), ("d_link_first", C.c_void_p), ("d_link_b", C.c_void_p)]


class UnitigsGfa(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_links", C.c_uint64), ("text_bytes", C.c_uint64), ("total_bases", C.c_uint64),
                ("longest", C.c_uint64), ("read_bytes", C.c_uint64), ("k", C.c_uint32), ("n_devices", C.c_uint32),
                ("shrink", DistShrinkStats)]


class DistStandardizeStats(C.Structure):
    _fields_ = [("route", C.c_uint32), ("rank_rounds", C.c_uint32), ("exchanges", C.c_uint64), ("contigs", C.c_uint64),
                ("longest_contig", C.c_uint64), ("cycle_edges", C.c_uint64), ("bytes_sent", C.c_uint64)]


# the caller's transport (katome_comm_callbacks)
A2A_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, u64p, u64p, C.c_void_p, u64p, u64p, C.c_uint64, C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, u64p, C.c_uint64, C.c_int)


class CommCallbacks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("alltoallv", A2A_FN), ("allreduce_u64", ALLREDUCE_FN)]


# every symbol include/katome_gpu.h declares: name -> (restype, argtypes)
_vp, _sz, _i, _u32, _u64, _dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64, C.c_double
_pp = C.POINTER(C.c_char_p)
SYMBOLS = {
    "katome_build_files": (_i, [C.POINTER(Settings), _pp, _sz, C.POINTER(C.POINTER(Graph))]),
    "katome_build_files_staged": (_i, [C.POINTER(Settings), _pp, _sz, C.c_char_p, _u64, C.POINTER(C.POINTER(Graph))]),
    "katome_build_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.POINTER(C.POINTER(Graph))]),
    "katome_build_packed_staged": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.c_char_p, _u64, C.POINTER(C.POINTER(Graph))]),
    "katome_build_files_staged_stats": (_i, [C.POINTER(Settings), _pp, _sz, C.c_char_p, _u64, C.POINTER(Stats), C.POINTER(C.POINTER(Graph))]),
    "katome_build_packed_staged_stats": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.c_char_p, _u64, C.POINTER(Stats),
                                         C.POINTER(C.POINTER(Graph))]),
    "katome_graph_free": (None, [C.POINTER(Graph)]),
    "katome_graph_stats": (_i, [C.POINTER(Graph), C.POINTER(Stats)]),
    "katome_last_error": (C.c_char_p, []),
    "katome_abi_version": (_u32, []),
    "katome_ingest_files": (_i, [C.POINTER(Settings), _pp, _sz, C.POINTER(C.POINTER(Reads))]),
    "katome_reads_free": (None, [C.POINTER(Reads)]),
    "katome_builder_create": (_i, [C.POINTER(Settings), C.POINTER(_vp)]),
    "katome_builder_destroy": (None, [_vp]),
    "katome_record_words": (_u32, [_u32]),
    "katome_builder_counts": (_i, [_vp, u64p]),
    "katome_builder_profile": (_i, [_vp, _i]),
    "katome_builder_profile_read": (_i, [_vp, C.POINTER(_dbl), u64p]),
    "katome_builder_profile_read_work": (_i, [_vp, C.POINTER(_dbl), u64p, u64p]),
    "katome_phase_count": (_u32, []),
    "katome_phase_name": (C.c_char_p, [_u32]),
    "katome_dev_extract_fixed": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp]),
    "katome_dev_extract_var": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    "katome_dev_extract_var_tiles": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u32, _vp, _vp]),
    "katome_dev_extract_var_remainder": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u32, _vp, _vp]),
    "katome_dev_partition": (_i, [_i, _vp, _vp, _u64, _u32, _u32, _vp, _vp, u64p, _vp]),
    "katome_dev_partition_core": (_i, [_i, _vp, _vp, _u64, _u32, _u32, _u32, _u32, _vp, _vp, u64p, _vp]),
    "katome_key_owner": (_u32, [u64p, _u32, _u32, _u32, _u32]),
    "katome_dev_source_ids": (_i, [_i, _vp, _u64, _u32, _vp, _vp, u64p, _vp]),
    "katome_dev_insert": (_i, [_vp, _vp, _u64, _vp]),
    "katome_dev_insert_weighted": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "katome_dev_remove_weak_edges": (_i, [_vp, _u32, _vp]),
    "katome_dev_table_count": (_i, [_vp, u64p, _vp]),
    "katome_tile_span": (_u32, [_u32, _u32]),
    "katome_tile_words": (_u32, [_u32, _u32]),
    "katome_tile_plan": (_u32, [_u32, _u32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "katome_tile_plan_limited": (_u32, [_u32, _u32, _u32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "katome_tile_span_for_lengths": (_u32, [_u32, C.POINTER(C.c_uint32), _u64]),
    "katome_dev_extract_remainder": (_i, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp]),
    "katome_dev_extract_tiles": (_i, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp]),
    "katome_dev_insert_tiles": (_i, [_vp, _vp, _u64, _u32, _vp]),
    "katome_dev_count_tiles": (_i, [_vp, _vp, _u64, _u32, _u32, _vp, _vp]),
    "katome_dev_expand_tiles": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), u64p, _vp]),
    "katome_dev_finalize": (_i, [_vp, C.POINTER(DevGraph), _vp]),
    "katome_shrink_files": (_i, [C.POINTER(Settings), _pp, _sz, C.POINTER(C.POINTER(Contigs))]),
    "katome_shrink_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.POINTER(C.POINTER(Contigs))]),
    "katome_contigs_free": (None, [C.POINTER(Contigs)]),
    "katome_dev_standardize_contigs": (_i, [_vp, _vp]),
    "katome_dev_standardize_edges": (_i, [_vp, _u64, _u32, _vp]),
    "katome_dev_shrink": (_i, [_vp, C.POINTER(DevContigs), _vp]),
    "katome_dev_shrink_mode": (_i, [_vp, C.c_uint32, C.POINTER(DevContigs), C.POINTER(C.c_double), _vp]),
    "katome_dev_shrink_coverage": (_i, [_vp, C.c_uint32, C.POINTER(DevContigs), C.POINTER(DevCoverage), C.POINTER(C.c_double), _vp]),
    "katome_dev_depth": (_i, [_vp, _u32, _u32, _vp, _u64, _vp, _vp, _u64, C.POINTER(DevDepth), _vp]),
    "katome_dev_depth_index_bytes": (_u64, [_vp]),
    "katome_depth_paths": (_i, [C.POINTER(Settings), _pp, _sz, C.c_char_p, _u64, _pp, _sz, _u32, _u32, C.POINTER(C.POINTER(Depth))]),
    "katome_depth_free": (None, [C.POINTER(Depth)]),
    "katome_dev_depth_arrays": (_i, [_i, _u32, _vp, _vp, _u64, _u32, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, u64p, _vp]),
    "katome_dev_collapse": (_i, [_vp, _u32, C.POINTER(DevAssembly), C.POINTER(CollapseStats), _vp]),
    "katome_dev_contigs_text": (_i, [_vp, C.POINTER(DevContigs), _u32, C.POINTER(DevAssembly), _vp]),
    "katome_dev_pieces_text": (_i, [_i, _u32, _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _vp, _u64, u64p, u64p, _vp]),
    "katome_dev_pieces_text_numbered": (_i, [_i, _u32, _vp, _vp, _u64, _vp, _u64, _u32, _u64, _vp, _vp, _u64, _vp, _u64, u64p, u64p, _vp]),
    "katome_dev_contigs_gfa": (_i, [_vp, C.POINTER(DevContigs), C.POINTER(DevGfa), _vp]),
    "katome_dev_gfa_arrays": (_i, [_i, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, u64p, u64p, _vp]),
    "katome_dev_contigs_gfa_coverage": (_i, [_vp, C.POINTER(DevContigs), C.POINTER(DevGfa), _vp]),
    "katome_dev_gfa_coverage_arrays": (_i, [_i, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, u64p, u64p, _vp]),
    "katome_dev_gfa_part_arrays": (_i, [_i, _u32, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _i, _vp, _vp, _vp, _vp, _u64, u64p, u64p, u64p, _vp]),
    "katome_gfa_files": (_i, [C.POINTER(Settings), _pp, _sz, C.c_char_p, _u64, C.c_char_p, C.POINTER(C.POINTER(Gfa))]),
    "katome_gfa_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.c_char_p, _u64, C.c_char_p, C.POINTER(C.POINTER(Gfa))]),
    "katome_gfa_save": (_i, [C.POINTER(Gfa), C.c_char_p]),
    "katome_gfa_free": (None, [C.POINTER(Gfa)]),
    "katome_dev_contigs_gfa_strands": (_i, [_vp, C.POINTER(DevContigs), C.POINTER(DevGfaStrands), _vp]),
    "katome_dev_gfa_strands_arrays": (_i, [_i, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, u64p, _vp]),
    "katome_gfa_strands_files": (_i, [C.POINTER(Settings), _pp, _sz, C.c_char_p, _u64, C.c_char_p, C.POINTER(C.POINTER(GfaStrands))]),
    "katome_gfa_strands_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.c_char_p, _u64, C.c_char_p, C.POINTER(C.POINTER(GfaStrands))]),
    "katome_gfa_strands_save": (_i, [C.POINTER(GfaStrands), C.c_char_p]),
    "katome_gfa_strands_free": (None, [C.POINTER(GfaStrands)]),
    "katome_unitigs_files": (_i, [C.POINTER(Settings), _pp, _sz, C.c_char_p, _u64, C.c_char_p, C.POINTER(Unitigs)]),
    "katome_unitigs_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.c_char_p, _u64, C.c_char_p, C.POINTER(Unitigs)]),
    "katome_unitigs_gfa_files": (_i, [C.POINTER(Settings), _pp, _sz, C.c_char_p, _u64, C.c_char_p, C.POINTER(UnitigsGfa)]),
    "katome_unitigs_gfa_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, C.c_char_p, _u64, C.c_char_p, C.POINTER(UnitigsGfa)]),
    "katome_dev_collapse_gfa": (_i, [_vp, C.POINTER(DevGfaPaths), _vp]),
    "katome_dev_gfa_paths_arrays": (_i, [_i, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64, u64p, _vp]),
    "katome_assemble_gfa_files": (_i, [C.POINTER(Settings), _pp, _sz, _u64, C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(Assembly)),
                                  C.POINTER(C.POINTER(GfaPaths))]),
    "katome_assemble_gfa_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, _u64, C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(Assembly)),
                                   C.POINTER(C.POINTER(GfaPaths))]),
    "katome_gfa_paths_save": (_i, [C.POINTER(GfaPaths), C.c_char_p]),
    "katome_gfa_paths_free": (None, [C.POINTER(GfaPaths)]),
    "katome_dev_collapse_gfa_strands": (_i, [_vp, C.POINTER(DevGfaStrandPaths), _vp]),
    "katome_dev_gfa_strand_paths_arrays": (_i, [_i, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _u64, u64p, _vp]),
    "katome_dev_collapse_unique": (_i, [_vp, _u32, C.POINTER(DevUniqueAssembly), _vp]),
    "katome_dev_unique_contigs_arrays": (_i, [_i, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64, u64p, _vp]),
    "katome_assemble_unique_files": (_i, [C.POINTER(Settings), _pp, _sz, _u64, C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(Assembly)),
                                     C.POINTER(C.POINTER(UniqueAssembly))]),
    "katome_assemble_unique_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, _u64, C.c_char_p, C.c_char_p,
                                      C.POINTER(C.POINTER(Assembly)), C.POINTER(C.POINTER(UniqueAssembly))]),
    "katome_unique_assembly_save": (_i, [C.POINTER(UniqueAssembly), C.c_char_p]),
    "katome_unique_assembly_free": (None, [C.POINTER(UniqueAssembly)]),
    "katome_assemble_gfa_strands_files": (_i, [C.POINTER(Settings), _pp, _sz, _u64, C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(Assembly)),
                                          C.POINTER(C.POINTER(GfaStrandPaths))]),
    "katome_assemble_gfa_strands_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, _u64, C.c_char_p, C.c_char_p,
                                           C.POINTER(C.POINTER(Assembly)), C.POINTER(C.POINTER(GfaStrandPaths))]),
    "katome_gfa_strand_paths_save": (_i, [C.POINTER(GfaStrandPaths), C.c_char_p]),
    "katome_gfa_strand_paths_free": (None, [C.POINTER(GfaStrandPaths)]),
    "katome_contig_stats_of": (_i, [u64p, _u64, _u64, C.POINTER(ContigStats)]),
    "katome_assemble_files": (_i, [C.POINTER(Settings), _pp, _sz, _u64, C.c_char_p, C.POINTER(C.POINTER(Assembly))]),
    "katome_assemble_packed": (_i, [C.POINTER(Settings), _vp, _u64, _u32, _vp, _u64, C.c_char_p, C.POINTER(C.POINTER(Assembly))]),
    "katome_assembly_save": (_i, [C.POINTER(Assembly), C.c_char_p]),
    "katome_assembly_free": (None, [C.POINTER(Assembly)]),
    "katome_dev_current_graph": (_i, [_vp, C.POINTER(DevGraph)]),
    "katome_dev_graph_stats": (_i, [_vp, C.POINTER(Stats), _vp]),
    "katome_dev_weight_spectrum": (_i, [_vp, u64p, _u32, _vp]),
    "katome_dev_stats_arrays": (_i, [_i, _vp, _vp, _vp, _u64, _u64, C.POINTER(Stats), _vp]),
    "katome_dev_weight_spectrum_arrays": (_i, [_i, _vp, _u64, u64p, _u32, _vp]),
    "katome_dev_scan_counts": (_i, [_i, _vp, _u64, _vp, _vp]),
    "katome_dev_replay_node_removals": (_i, [_i, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "katome_dev_replay_edge_removals": (_i, [_i, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "katome_dev_replay_node_removals64": (_i, [_i, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "katome_dev_replay_edge_removals64": (_i, [_i, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "katome_dev_remove_dead_paths": (_i, [_vp, C.POINTER(DevGraph), C.POINTER(PruneStats), _vp]),
    "katome_dev_edges": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), u64p, _vp]),
    "katome_dev_release_cache": (_i, [_i]),
    "katome_dev_cache_stats": (_i, [_i, u64p]),
    "katome_dev_sort": (_i, [_i, _vp, _vp, _u64, _u32, _u32, _vp]),
    "katome_dev_list_first_pass": (_i, [_i, _vp, _vp, _u64, _u32, _u32, _u32, _u32, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "katome_dev_count_in_key": (_i, [_i, _vp, _vp, _u64, _u32, _u32, _u32, _u32, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, u64p, C.POINTER(C.c_int), _vp]),
    "katome_dev_count_records": (_i, [_i, _vp, _vp, _u64, _u32, _i, _u32, _u32, _vp, _vp, _u64, u64p, u64p, u64p, u64p, _vp]),
    "katome_s2_region_starts": (None, [u64p, u64p]),
    "katome_dev_s2_region_pass": (_i, [_i, _u32, u64p, _vp, _vp, _vp, _vp, _vp, _vp]),
    "katome_dev_unique": (_i, [_i, _vp, _u64, _u32, u64p, _vp]),
    "katome_dev_rank": (_i, [_i, _vp, _u64, _u32, _u32, _vp, _u64, _vp, _vp]),
    "katome_dev_node_ids": (_i, [_i, _vp, _u64, _u32, _vp, _vp, _vp, u64p, _vp]),
    "katome_dev_endpoints": (_i, [_i, _vp, _u64, _u32, _vp, _vp, _vp]),
    "katome_dev_labels": (_i, [_i, _vp, _u64, _u32, _vp, _vp]),
    "katome_dev_synth_reads": (_i, [_i, _u64, _u64, _u32, _u64, _dbl, _u32, _vp, _vp, _vp]),
    # multi-GPU: communicators and the sharded build
    "katome_comm_unique_id": (_i, [_vp]),
    "katome_comm_create_rccl": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "katome_comm_create_callbacks": (_i, [C.POINTER(CommCallbacks), _i, _i, _i, C.POINTER(_vp)]),
    "katome_comm_destroy": (None, [_vp]),
    "katome_comm_rank": (_i, [_vp]),
    "katome_comm_world": (_i, [_vp]),
    "katome_comm_kind": (C.c_char_p, [_vp]),
    "katome_comm_set_max_message_bytes": (_i, [_vp, _u64]),
    "katome_comm_allreduce_u64": (_i, [_vp, u64p, _u64, _i]),
    "katome_comm_exchange": (_i, [_vp, _vp, u64p, _vp, _u64, u64p, _u64, _i, _vp]),
    "katome_dist_create": (_i, [C.POINTER(Settings), _vp, C.POINTER(_vp)]),
    "katome_dist_destroy": (None, [_vp]),
    "katome_dist_add_reads": (_i, [_vp, _vp, _u64, _u64, _u32, _vp, _u64, _vp]),
    "katome_dist_add_reads_var": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _u64, _u64, _vp]),
    "katome_dist_remove_weak_edges": (_i, [_vp, _u32]),
    "katome_dist_finalize": (_i, [_vp, C.POINTER(DistGraph), _vp]),
    "katome_dist_gather": (_i, [_vp, _i, C.POINTER(_vp), _vp]),
    "katome_dist_inner": (_vp, [_vp]),
    "katome_dist_route": (C.c_char_p, [_vp]),
    "katome_dist_remove_dead_paths": (_i, [_vp, C.POINTER(DistGraph), C.POINTER(PruneStats), _vp]),
    "katome_dist_current_graph": (_i, [_vp, C.POINTER(DistGraph)]),
    "katome_dist_standardize_contigs": (_i, [_vp, C.POINTER(DistGraph), _vp]),
    "katome_dist_standardize_stats_read": (_i, [_vp, C.POINTER(DistStandardizeStats)]),
    "katome_dist_prune_weak_edges": (_i, [_vp, C.c_uint32, C.POINTER(DistGraph), _vp]),
    "katome_dist_standardize_edges": (_i, [_vp, C.c_uint64, C.c_uint32, C.POINTER(DistGraph), _vp]),
    "katome_dist_shrink": (_i, [_vp, C.POINTER(DistContigs), C.POINTER(DistShrinkStats), _vp]),
    "katome_dist_shrink_coverage": (_i, [_vp, C.POINTER(DistContigs), C.POINTER(DevCoverage), C.POINTER(DistShrinkStats), _vp]),
    "katome_dist_contigs_text": (_i, [_vp, _u32, C.POINTER(DistAssembly), _vp]),
    "katome_dist_contig_stats_arrays": (_i, [_vp, _i, _vp, _u64, _u32, _u64, C.POINTER(ContigStats), _vp]),
    "katome_dist_contig_stats": (_i, [_vp, _u64, C.POINTER(ContigStats), _vp]),
    "katome_dist_contigs_save": (_i, [_vp, C.POINTER(DistAssembly), C.c_char_p]),
    "katome_dist_contigs_gfa": (_i, [_vp, C.POINTER(DistGfa), _vp]),
    "katome_dist_contigs_gfa_coverage": (_i, [_vp, C.POINTER(DistGfa), _vp]),
    "katome_dist_gfa_save": (_i, [_vp, C.POINTER(DistGfa), C.c_char_p]),
    "katome_dist_graph_stats": (_i, [_vp, C.POINTER(Stats), _vp]),
    "katome_dist_weight_spectrum": (_i, [_vp, u64p, _u32, _vp]),
    "katome_dist_exchange_count": (_u32, []),
    "katome_dist_exchange_name": (C.c_char_p, [_u32]),
    "katome_dist_exchange_read": (_i, [_vp, u64p]),
    "katome_shard_range": (None, [_u64, _u32, _u32, u64p, u64p]),
}


# test entries that the library of an older commit, loaded with KATOME_LIB for an A/B of the benchmark, does not have: that library
# loads without them (and a test that calls one fails on the missing attribute); every other symbol must be there
_TEST_ENTRIES_AFTER_AB = {"katome_dev_count_in_key", "katome_dev_count_records"}
# public entries that the library of the commit before them lacks and the benchmark does not call: passed over ONLY in a library
# named by KATOME_LIB -- the tree's own library must have every symbol
_ENTRIES_AFTER_AB = {"katome_dev_depth", "katome_dev_depth_index_bytes", "katome_dev_depth_arrays", "katome_depth_paths", "katome_depth_free"}


def lib_path():
    return os.environ.get("KATOME_LIB") or os.path.join(_HERE, "lib", "libkatome_gpu.so")


def lib():
    """Load the HIP library.  Fails loudly when it has not been built: there is no fallback."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C katome_amd/csrc` (no CPU fallback exists)" % path)
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            if name in _TEST_ENTRIES_AFTER_AB and not hasattr(L, name):
                continue
            if name in _ENTRIES_AFTER_AB and os.environ.get("KATOME_LIB") and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def last_error():
    return lib().katome_last_error().decode(errors="replace")
