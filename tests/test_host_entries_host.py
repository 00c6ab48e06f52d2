"""No-GPU characterisation of the host entries of include/katome_gpu.h (katome_amd/csrc/host_build.cpp): every ending exists as
a `_files` and a `_packed` twin, and both refuse the same bad arguments, in the same order and with the same message, before a
device is asked for.  Also every katome_*_free(NULL) and every katome_*_save on a struct made by hand."""
import ctypes as C
import os

import numpy as np
import pytest

import katome_amd
from katome_amd import _lib
from katome_amd.build import InputFileType, make_settings

E_PATH, E_OPEN, E_ARG, E_DEVICE, E_UNSUPPORTED = -1, -4, -7, -8, -10
NEED_ORDER = "stages after the build need KATOME_FLAG_FIRST_SEEN_ORDER"
UNITIGS_NEED_ORDER = "unitigs: stage letters and KATOME_FLAG_REMOVE_DEAD_PATHS need KATOME_FLAG_FIRST_SEEN_ORDER"

# every pair: the symbol (with the twin's word left open) and what follows the reads in its argument list.  "stages", "genome",
# "path" and "stats" are inputs; a ctypes Structure class is a `T** out` the library owns; ("struct", T) is a plain `T* out`.
ENTRIES = {
    "build": ("katome_build_{}", [_lib.Graph]),
    "staged": ("katome_build_{}_staged", ["stages", "genome", _lib.Graph]),
    "staged_stats": ("katome_build_{}_staged_stats", ["stages", "genome", "stats", _lib.Graph]),
    "assemble": ("katome_assemble_{}", ["genome", "path", _lib.Assembly]),
    "assemble_gfa": ("katome_assemble_gfa_{}", ["genome", "path", "path", _lib.Assembly, _lib.GfaPaths]),
    "assemble_gfa_strands": ("katome_assemble_gfa_strands_{}", ["genome", "path", "path", _lib.Assembly, _lib.GfaStrandPaths]),
    "assemble_unique": ("katome_assemble_unique_{}", ["genome", "path", "path", _lib.Assembly, _lib.UniqueAssembly]),
    "unitigs": ("katome_unitigs_{}", ["stages", "genome", "path", ("struct", _lib.Unitigs)]),
    "unitigs_gfa": ("katome_unitigs_gfa_{}", ["stages", "genome", "path", ("struct", _lib.UnitigsGfa)]),
    "gfa": ("katome_gfa_{}", ["stages", "genome", "path", _lib.Gfa]),
    "gfa_strands": ("katome_gfa_strands_{}", ["stages", "genome", "path", _lib.GfaStrands]),
    "shrink": ("katome_shrink_{}", [_lib.Contigs]),
}
TWINS = ("files", "packed")
PAIRS = [(name, twin) for name in ENTRIES for twin in TWINS]


def test_the_table_names_every_pair_of_the_header():
    twins = sorted(n for n in _lib.SYMBOLS if n.split("_")[-1] in TWINS or "_files_" in n or "_packed_" in n)
    twins.remove("katome_ingest_files")
    assert twins == sorted(fmt.format(twin) for fmt, _ in ENTRIES.values() for twin in TWINS)


class Call:
    """one call of an entry: the reads of the twin in front, then the entry's own arguments; `null_out`: every result pointer
    and every path NULL, else every `T** out` points at a non-NULL pointer and every plain struct is filled with 0xFF"""

    def __init__(self, name, twin, settings, golden_dir, stages=b"", null_out=False, files=None):
        fmt, tail = ENTRIES[name]
        self.fn = getattr(katome_amd.lib(), fmt.format(twin))
        self.pointers, self.structs, self.keep = [], [], []
        s = C.byref(settings) if settings is not None else None
        if twin == "files":
            files = files or [os.path.join(golden_dir, "data1.txt")]
            self.args = [s, (C.c_char_p * len(files))(*[os.fsencode(f) for f in files]), len(files)]
        else:
            packed = np.zeros(38, np.uint8)
            self.keep.append(packed)
            self.args = [s, packed.ctypes.data, 1, 150, None]
        for what in tail:
            if what == "stages":
                self.args.append(stages)
            elif what == "genome":
                self.args.append(1000)
            elif what == "path":
                self.args.append(None)
            elif what == "stats":
                self.args.append(None if null_out else (_lib.Stats * (len(stages) + 1))())
            elif isinstance(what, tuple):
                st = what[1]()
                C.memset(C.byref(st), 0xFF, C.sizeof(st))
                self.structs.append(st)
                self.args.append(None if null_out else C.byref(st))
            else:
                target = what()
                self.keep.append(target)
                p = C.POINTER(what)(target)
                assert p
                self.pointers.append(p)
                self.args.append(None if null_out else C.byref(p))

    def __call__(self):
        return self.fn(*self.args), _lib.last_error()

    def outputs_cleared(self):
        return all(not p for p in self.pointers) and all(bytes(st) == bytes(C.sizeof(st)) for st in self.structs)


def settings_for(twin, **kw):
    return make_settings(40, InputFileType.Fastq, **kw) if twin == "files" else make_settings(31, **kw)


@pytest.mark.parametrize("name,twin", PAIRS)
def test_no_result_pointer_and_no_path_is_a_null_argument(golden_dir, name, twin):
    assert Call(name, twin, settings_for(twin, first_seen_order=True), golden_dir, null_out=True)() == (E_ARG, "null argument")


@pytest.mark.parametrize("name,twin", PAIRS)
def test_null_settings_clear_the_outputs_first(golden_dir, name, twin):
    call = Call(name, twin, None, golden_dir)
    assert call() == (E_ARG, "null argument")
    assert call.outputs_cleared()


@pytest.mark.parametrize("name,twin", PAIRS)
def test_k_64(golden_dir, name, twin):
    s = settings_for(twin, first_seen_order=True)
    s.k = 64
    call = Call(name, twin, s, golden_dir)
    if twin == "packed":
        assert call() == (E_UNSUPPORTED, "k = 64 unsupported (3..63)")
    else:                                   # (the files twins meet k in the ingest: whatever katome_ingest_files answers)
        rp = C.POINTER(_lib.Reads)()
        want = katome_amd.lib().katome_ingest_files(*call.args[:3], C.byref(rp)), _lib.last_error()
        assert want[0] != 0 and not rp
        assert call() == want
    assert call.outputs_cleared()


@pytest.mark.parametrize("name", ["gfa", "gfa_strands"])
@pytest.mark.parametrize("twin", TWINS)
def test_gfa_refuses_stage_letters_without_first_seen_order(golden_dir, name, twin):
    call = Call(name, twin, settings_for(twin), golden_dir, stages=b"dc")
    assert call() == (E_ARG, NEED_ORDER)
    assert call.outputs_cleared()


@pytest.mark.parametrize("name", ["unitigs", "unitigs_gfa"])
@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("stages,dead_paths", [(b"dc", False), (b"", True), (b"w", True)])
def test_unitigs_refuse_pruning_without_first_seen_order(golden_dir, name, twin, stages, dead_paths):
    call = Call(name, twin, settings_for(twin, remove_dead_paths=dead_paths), golden_dir, stages=stages)
    assert call() == (E_ARG, UNITIGS_NEED_ORDER)
    assert call.outputs_cleared()           # (the caller's struct came in as 0xFF bytes)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_missing_file_is_found_before_any_device(golden_dir, name):
    call = Call(name, "files", settings_for("files", first_seen_order=True), golden_dir,
                files=[os.path.join(golden_dir, "no_such_reads.txt")])
    assert call()[0] == E_PATH
    assert call.outputs_cleared()


@pytest.mark.parametrize("name,twin", PAIRS)
def test_without_a_device_every_entry_fails_loudly(golden_dir, name, twin):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    call = Call(name, twin, settings_for(twin, first_seen_order=True), golden_dir)
    rc, message = call()
    assert rc == E_DEVICE and "no CPU fallback" in message
    assert call.outputs_cleared()


def test_every_free_takes_null():
    frees = sorted(n for n in _lib.SYMBOLS if n.endswith("_free"))
    assert len(frees) >= 9
    for name in frees:
        assert getattr(katome_amd.lib(), name)(None) is None


# ---- katome_*_save: the struct made by hand, its text a numpy buffer -------------------------------------------------------------
SAVES = {                                   # symbol -> (struct, the file is text[:text_bytes + path_bytes])
    "katome_assembly_save": (_lib.Assembly, False),
    "katome_unique_assembly_save": (_lib.UniqueAssembly, False),
    "katome_gfa_save": (_lib.Gfa, False),
    "katome_gfa_strands_save": (_lib.GfaStrands, False),
    "katome_gfa_paths_save": (_lib.GfaPaths, True),
    "katome_gfa_strand_paths_save": (_lib.GfaStrandPaths, True),
}
TEXT_FASTA = 1


def hand_made(name, text_bytes=41, path_bytes=17):
    """-> (struct, its text buffer with 7 bytes after the end that no file may hold, the bytes the file must hold)"""
    cls, with_paths = SAVES[name]
    text = np.frombuffer(bytes((37 * i + 11) % 251 for i in range(text_bytes + path_bytes + 7)), np.uint8).copy()
    st = cls()
    st.text_bytes = text_bytes
    st.text = text.ctypes.data_as(_lib.u8p)
    if with_paths:
        st.path_bytes = path_bytes
    if cls is _lib.Assembly:
        st.layout = TEXT_FASTA
    return st, text, bytes(text[:text_bytes + (path_bytes if with_paths else 0)])


def test_the_table_names_every_save():
    assert sorted(SAVES) == sorted(n for n in _lib.SYMBOLS if n.endswith("_save") and not n.startswith("katome_dist_"))


@pytest.mark.parametrize("name", list(SAVES))
def test_save_writes_exactly_the_text(tmp_path, name):
    fn = getattr(katome_amd.lib(), name)
    st, text, want = hand_made(name)
    path = tmp_path / "out.txt"
    assert fn(C.byref(st), os.fsencode(str(path))) == 0
    assert path.read_bytes() == want
    st, text, want = hand_made(name, text_bytes=0, path_bytes=0)      # an empty text is an empty file
    assert fn(C.byref(st), os.fsencode(str(path))) == 0
    assert path.read_bytes() == b""


@pytest.mark.parametrize("name", list(SAVES))
def test_save_refuses_null_and_reports_a_path_it_cannot_create(tmp_path, name):
    fn = getattr(katome_amd.lib(), name)
    st, text, _ = hand_made(name)
    path = tmp_path / "out.txt"
    assert (fn(None, os.fsencode(str(path))), _lib.last_error()) == (E_ARG, "null argument")
    assert (fn(C.byref(st), None), _lib.last_error()) == (E_ARG, "null argument")
    assert not path.exists()
    missing = str(tmp_path / "no_such_dir" / "out.txt")
    assert (fn(C.byref(st), os.fsencode(missing)), _lib.last_error()) == (E_OPEN, "couldn't create %s: entity not found" % missing)


def test_assembly_save_refuses_a_text_that_is_not_fasta(tmp_path):
    st, text, _ = hand_made("katome_assembly_save")
    st.layout = 0
    path = tmp_path / "out.txt"
    assert katome_amd.lib().katome_assembly_save(C.byref(st), os.fsencode(str(path))) == E_ARG
    assert _lib.last_error() == "assembly_save: the text is not in FASTA layout"
    assert not path.exists()
