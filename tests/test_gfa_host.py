"""No-GPU checks of the GFA export: the Python model of the format (tests/gfa_model.py) against three GFA texts written out by
hand, and the host entries katome_gfa_* failing loudly (E_DEVICE, no CPU fallback) on a box without a GPU."""
import os

import numpy as np
import pytest

import gfa_model
from katome_amd.build import GpuGraph, InputFileType, KatomePanic, set_global_k_sizes


def test_model_no_edges():
    text, seg, first = gfa_model.gfa_text(5, [], [], [], [], [])
    assert text == b"H\tVN:Z:1.0\n" and seg == [] and first == [0]
    assert gfa_model.parse(text) == ([], [])


def test_model_chain_with_a_self_loop():
    """0 -> 1 -> 2 with a loop on vertex 1: k = 3, so labels are kmers + 2 bases and the overlap is 2M"""
    #        edge 0: 0 -> 1      edge 1: 1 -> 1 (loop)   edge 2: 1 -> 2
    src, dst = [0, 1, 1], [1, 1, 2]
    weight, kmers, seqs = [7, 1, 4000000000], [2, 1, 3], ["ACGT", "GTG", "GTGCA"]
    text, seg, first = gfa_model.gfa_text(3, src, dst, weight, kmers, seqs)
    want = ("H\tVN:Z:1.0\n"
            "S\t0\tACGT\tLN:i:4\tKC:i:14\tew:i:7\n"
            "S\t1\tGTG\tLN:i:3\tKC:i:1\tew:i:1\n"
            "S\t2\tGTGCA\tLN:i:5\tKC:i:12000000000\tew:i:4000000000\n"
            "L\t0\t+\t1\t+\t2M\n"
            "L\t0\t+\t2\t+\t2M\n"
            "L\t1\t+\t1\t+\t2M\n"
            "L\t1\t+\t2\t+\t2M\n").encode()
    assert text == want
    assert first == [0, 2, 4, 4]
    assert [text[o:o + len(s)].decode() for o, s in zip(seg, seqs)] == seqs
    segments, lks = gfa_model.parse(text)
    assert [s[1] for s in segments] == seqs and segments[2][2] == {"LN": 5, "KC": 12000000000, "ew": 4000000000}
    assert lks == [(0, 1, 2), (0, 2, 2), (1, 1, 2), (1, 2, 2)]


def test_model_shuffled_sources_and_parallel_edges():
    """edges listed in no source order, two parallel edges 2 -> 0, names of two digits: links by a, then b"""
    k = 11
    src = [2, 0, 2, 1] + [3] * 7
    dst = [0, 1, 0, 2] + [3] * 7
    seqs = ["ACGTACGTACG" + "T" * i for i in range(11)]
    kmers = [len(s) - k + 1 for s in seqs]
    weight = list(range(1, 12))
    text, seg, first = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)
    lines = text.decode().split("\n")
    assert lines[1] == "S\t0\tACGTACGTACG\tLN:i:11\tKC:i:1\tew:i:1"
    assert lines[11] == "S\t10\tACGTACGTACGTTTTTTTTTT\tLN:i:21\tKC:i:121\tew:i:11"
    assert lines[12:17] == ["L\t0\t+\t1\t+\t10M", "L\t1\t+\t3\t+\t10M", "L\t2\t+\t1\t+\t10M", "L\t3\t+\t0\t+\t10M", "L\t3\t+\t2\t+\t10M"]
    assert lines[17] == "L\t4\t+\t4\t+\t10M" and lines[23] == "L\t4\t+\t10\t+\t10M" and lines[-2] == "L\t10\t+\t10\t+\t10M"
    assert len(lines) == 1 + 11 + 5 + 49 + 1
    assert first[:5] == [0, 1, 2, 3, 5] and first[-1] == 54
    assert seg[10] - seg[9] == len(lines[10]) + 1 + 1           # (the name of segment 10 has one digit more)
    assert gfa_model.links(src, dst) == sorted(gfa_model.links(src, dst))
    raw = gfa_model.compress_edge(seqs[3])
    assert raw[0] == (4 - 14 % 4) % 4 and gfa_model.decompress_edge(raw) == seqs[3]


def test_no_gpu_means_loud_failure(golden_dir, tmp_path):
    """On a box without a GPU the GFA entries fail with E_DEVICE -- never a CPU path, and no file"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    set_global_k_sizes(40)
    out = str(tmp_path / "graph.gfa")
    with pytest.raises(KatomePanic) as e:
        GpuGraph.gfa([os.path.join(golden_dir, "data1.txt")], InputFileType.Fastq, False, 0, output_file=out)
    assert e.value.name == "E_DEVICE" and e.value.result is None and not os.path.exists(out)
    with pytest.raises(KatomePanic) as e:
        GpuGraph.gfa([os.path.join(golden_dir, "data1.txt")], InputFileType.Fastq, False, 0, stages="dcwced", original_genome_length=1000)
    assert e.value.name == "E_DEVICE"
    with pytest.raises(KatomePanic) as e:
        GpuGraph.gfa_from_packed(np.zeros(38, np.uint8), 1, 150, k=31)
    assert e.value.name == "E_DEVICE"
