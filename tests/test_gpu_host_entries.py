"""The host entries on a GPU: every ending exists as a `_files` and a `_packed` twin, and on the same reads the two hand back the
same result -- every field, array and text -- and write the same files.  (What each ending must hold is checked against the
oracle by the tests of that ending; this pins only that the twins agree.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, RC, THRESHOLD, GENOME = 12, True, 1, 20000      # (test_assemble_files' settings on this file)
STAGES = "dc"


def fields(obj):
    """the public data of a result object"""
    return {name: value for name, value in vars(obj).items() if not name.startswith("_")}


RESULTS = ("GpuGraph", "GpuContigs", "GpuUnitigs", "UnitigsGfa", "Assembly", "Gfa", "GfaStrands", "GfaPaths", "GfaStrandPaths", "UniqueAssembly")


def same(a, b, where):
    """a == b, all the way down: results field by field, arrays element by element with their type, texts byte for byte"""
    assert type(a) is type(b), where
    if type(a).__name__ in RESULTS:
        same(fields(a), fields(b), where)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for key in a:
            if not key.endswith("_ms"):                 # (wall times of the collapse walk)
                same(a[key], b[key], "%s.%s" % (where, key))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), where
    else:
        assert a == b, where                            # (numbers, texts, ContigsStats, CollectionStats)


def test_files_and_packed_twins_agree(golden_dir, tmp_path):
    from katome_amd.build import GpuContigs, GpuGraph, GpuUnitigs, InputFileType, ingest_files, set_global_k_sizes
    path = os.path.join(golden_dir, "data3.txt")
    set_global_k_sizes(K)
    r = ingest_files([path], InputFileType.Fastq, K)
    assert r["fixed_len"] == 100 and r["n_reads"] == 233
    files, packed = ([path], InputFileType.Fastq, RC), (r["packed"], r["n_reads"], r["fixed_len"])
    order = dict(first_seen_order=True)

    def out(name, twin):
        return str(tmp_path / ("%s_%s" % (twin, name)))

    # every pair: (what is compared, the call through the files twin, the call through the packed twin, the files each writes)
    pairs = {
        "build": (lambda t: GpuGraph.create(*files, THRESHOLD, **order),
                  lambda t: GpuGraph.create_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD, **order), []),
        "staged": (lambda t: GpuGraph.create(*files, THRESHOLD, stages=STAGES, original_genome_length=GENOME, **order),
                   lambda t: GpuGraph.create_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD, stages=STAGES,
                                                         original_genome_length=GENOME, **order), []),
        "staged_stats": (lambda t: GpuGraph.create(*files, THRESHOLD, stages=STAGES, original_genome_length=GENOME, stage_stats=True, **order),
                         lambda t: GpuGraph.create_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD, stages=STAGES,
                                                               original_genome_length=GENOME, stage_stats=True, **order), []),
        "assemble": (lambda t: GpuGraph.assemble(*files, THRESHOLD, GENOME, output_file=out("a.fa", t)),
                     lambda t: GpuGraph.assemble_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD,
                                                             original_genome_length=GENOME, output_file=out("a.fa", t)), ["a.fa"]),
        "unique": (lambda t: GpuGraph.assemble_unique(*files, THRESHOLD, GENOME, fasta_file=out("u.fa", t), unique_file=out("u.unique.fa", t)),
                   lambda t: GpuGraph.assemble_unique_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD,
                                                                  original_genome_length=GENOME, fasta_file=out("u.fa", t),
                                                                  unique_file=out("u.unique.fa", t)), ["u.fa", "u.unique.fa"]),
        "unitigs": (lambda t: GpuUnitigs.create(*files, THRESHOLD, output_file=out("unitigs.fa", t), stages=STAGES, original_genome_length=GENOME, **order),
                    lambda t: GpuUnitigs.create_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD,
                                                            output_file=out("unitigs.fa", t), stages=STAGES, original_genome_length=GENOME,
                                                            **order), ["unitigs.fa"]),
        "unitigs_gfa": (lambda t: GpuUnitigs.gfa(*files, THRESHOLD, output_file=out("unitigs.gfa", t), stages=STAGES, original_genome_length=GENOME, **order),
                        lambda t: GpuUnitigs.gfa_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD,
                                                             output_file=out("unitigs.gfa", t), stages=STAGES, original_genome_length=GENOME,
                                                             **order), ["unitigs.gfa"]),
        # (katome_shrink_packed's Python entry takes no threshold; nothing in the shrink reads it)
        "shrink": (lambda t: GpuContigs.create(*files, 0, **order), lambda t: GpuContigs.create_from_packed(*packed, reverse_complement=RC, **order), []),
    }
    for merge in (False, True):
        tag = "_strands" if merge else ""
        pairs["assemble_gfa" + tag] = (
            lambda t, merge=merge: GpuGraph.assemble_gfa(*files, THRESHOLD, GENOME, fasta_file=out("g%d.fa" % merge, t),
                                                         gfa_file=out("g%d.gfa" % merge, t), merge_strands=merge),
            lambda t, merge=merge: GpuGraph.assemble_gfa_from_packed(*packed, reverse_complement=RC, minimal_weight_threshold=THRESHOLD,
                                                                     original_genome_length=GENOME, fasta_file=out("g%d.fa" % merge, t),
                                                                     gfa_file=out("g%d.gfa" % merge, t), merge_strands=merge),
            ["g%d.fa" % merge, "g%d.gfa" % merge])
        pairs["gfa" + tag] = (
            lambda t, merge=merge: GpuGraph.gfa(*files, THRESHOLD, stages=STAGES, original_genome_length=GENOME, output_file=out("s%d.gfa" % merge, t),
                                                merge_strands=merge),
            lambda t, merge=merge: GpuGraph.gfa_from_packed(*packed, reverse_complement=RC, threshold=THRESHOLD, stages=STAGES,
                                                            original_genome_length=GENOME, output_file=out("s%d.gfa" % merge, t),
                                                            merge_strands=merge),
            ["s%d.gfa" % merge])
    assert len(pairs) == 12
    for name, (from_files, from_packed, written) in pairs.items():
        a, b = from_files("files"), from_packed("packed")
        same(a, b, name)
        for f in written:
            text = open(out(f, "files"), "rb").read()
            assert len(text) > 0 and text == open(out(f, "packed"), "rb").read(), (name, f)
        if name == "assemble":
            assert len(a.contigs) > 10 and a.stats.n50 > 0
        if name == "staged_stats":
            assert len(a[0].stage_stats) == len(STAGES) + 1
