"""No-GPU checks of the graph-stats and weight-spectrum entries (include/katome_gpu.h): they are exported and bound, argument
errors are decided before the device is touched, and without a device every one of them fails with E_DEVICE -- there is no
CPU answer."""
import ctypes as C
import os

import numpy as np
import pytest

import katome_amd
from katome_amd import _lib
from katome_amd.build import InputFileType, make_settings

NEW = ["katome_dev_stats_arrays", "katome_dev_weight_spectrum_arrays", "katome_dev_graph_stats", "katome_dev_weight_spectrum",
       "katome_dist_graph_stats", "katome_dist_weight_spectrum", "katome_build_files_staged_stats", "katome_build_packed_staged_stats"]
E_ARG, E_DEVICE = -7, -8


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_new_symbols_are_bound_and_exported():
    raw = C.CDLL(_lib.lib_path())
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(raw, name), name
    assert katome_amd.lib().katome_abi_version() == 2


def test_phase_names_are_appended():
    L = katome_amd.lib()
    names = [L.katome_phase_name(i).decode() for i in range(L.katome_phase_count())]
    assert names[:14] == ["extract", "region_order", "insert", "emit_edges", "sort_edges", "node_set", "rank", "labels", "insert_tiles",
                          "expand_tiles", "expand_mid_tiles", "first_seen_order", "remove_dead_paths", "shrink"]
    assert names.index("k:group_merge_kernel") < names.index("graph_stats") < names.index("weight_spectrum")
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("n_bins", [0, 1, 16385])
def test_bad_bin_counts_are_argument_errors_before_the_device(n_bins):
    L = katome_amd.lib()
    bins = (C.c_uint64 * 16400)()
    # (a device ordinal no box has: were the device asked first, the answer would be E_DEVICE, with or without a GPU)
    assert L.katome_dev_weight_spectrum_arrays(1 << 20, None, 0, bins, n_bins, None) == E_ARG
    assert "n_bins" in _lib.last_error()
    assert L.katome_dev_weight_spectrum_arrays(1 << 20, None, 0, None, 16, None) == E_ARG


def test_null_stage_stats_is_an_argument_error(golden_dir):
    L = katome_amd.lib()
    s = make_settings(31, first_seen_order=True)
    gp = C.POINTER(_lib.Graph)()
    packed = np.zeros(38, np.uint8)
    assert L.katome_build_packed_staged_stats(C.byref(s), packed.ctypes.data, 1, 150, None, b"dc", 1000, None, C.byref(gp)) == E_ARG
    paths = (C.c_char_p * 1)(os.fsencode(os.path.join(golden_dir, "data1.txt")))
    s = make_settings(40, InputFileType.Fastq, first_seen_order=True)
    assert L.katome_build_files_staged_stats(C.byref(s), paths, 1, b"dc", 1000, None, C.byref(gp)) == E_ARG
    assert not gp


def test_no_gpu_means_no_answer(golden_dir):
    if not _no_gpu():
        pytest.skip("GPU present")
    L = katome_amd.lib()
    st = _lib.Stats()
    st.node_count = 77
    assert L.katome_dev_stats_arrays(0, None, None, None, 0, 5, C.byref(st), None) == E_DEVICE
    assert st.node_count == 77                                  # nothing was computed on the host
    bins = (C.c_uint64 * 16)()
    assert L.katome_dev_weight_spectrum_arrays(0, None, 0, bins, 16, None) == E_DEVICE
    stage = (_lib.Stats * 3)()
    gp = C.POINTER(_lib.Graph)()
    s = make_settings(31, first_seen_order=True)
    packed = np.zeros(38, np.uint8)
    assert L.katome_build_packed_staged_stats(C.byref(s), packed.ctypes.data, 1, 150, None, b"dc", 1000, stage, C.byref(gp)) == E_DEVICE
    paths = (C.c_char_p * 1)(os.fsencode(os.path.join(golden_dir, "data1.txt")))
    s = make_settings(40, InputFileType.Fastq, first_seen_order=True)
    assert L.katome_build_files_staged_stats(C.byref(s), paths, 1, b"dc", 1000, stage, C.byref(gp)) == E_DEVICE
    assert not gp and stage[0].edge_count == 0


def test_python_entries_take_stage_stats(golden_dir):
    """GpuGraph.create(..., stage_stats=True) goes through the new entry (here: as far as the missing device)"""
    if not _no_gpu():
        pytest.skip("GPU present")
    from katome_amd.build import GpuGraph, KatomePanic, set_global_k_sizes
    set_global_k_sizes(40)
    with pytest.raises(KatomePanic) as e:
        GpuGraph.create([os.path.join(golden_dir, "data1.txt")], InputFileType.Fastq, False, 0, first_seen_order=True, stages="d",
                        stage_stats=True)
    assert e.value.name == "E_DEVICE"
    with pytest.raises(KatomePanic) as e:
        GpuGraph.create_from_packed(np.zeros(38, np.uint8), 1, 150, k=31, stage_stats=True)
    assert e.value.name == "E_DEVICE"
