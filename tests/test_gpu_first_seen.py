"""The two routes to first-seen order (first_seen.hip): node indices as a running count over the edges in sequence order (the
default) and the nodes sorted by their first touch (KATOME_SORT_NODES) -- byte for byte against each other and against the oracle's
petgraph numbering, with one-word and with two-word keys (test_round_one_paths_give_the_same_arrays compares them at k = 31 only,
so the two-word forms of the pack / unpack / assign kernels and of the node-key gather had nothing to be compared with)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_build import _assert_same_as_reference_order  # noqa: E402

N_READS, READ_LEN, GENOME, ERR = 300, 60, 3000, 3e-3
ARRAYS = ("edge_key", "edge_weight", "edge_src", "edge_dst", "node_key", "edge_label")

_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from katome_amd import device as kd
k, rc, n, L = int(sys.argv[2]), sys.argv[3] == "1", int(sys.argv[4]), int(sys.argv[5])
reads = np.load(sys.argv[6])
packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
b = kd.Builder(k, rc, first_seen_order=True, table_slots_hint=1 << 16)
b.count_reads(packed, n, L, None, first_read=0)
dg = b.finalize()
np.savez(sys.argv[7], n_nodes=dg.n_nodes, n_edges=dg.n_edges,
         **{a: getattr(dg, a).cpu().numpy() for a in ("edge_key", "edge_weight", "edge_src", "edge_dst", "node_key", "edge_label")})
b.close()
"""


@pytest.mark.parametrize("k,rc", [(31, True), (41, False)])
def test_both_first_seen_routes_give_the_reference_order(oracle, tmp_path, k, rc):
    """each route in a process of its own (the switch is read once); several 256-thread blocks of edges, and read ends that
    leave nodes without out-edges, whose first touches the merge does not mark"""
    reads = oracle.synth_reads(0, N_READS, READ_LEN, GENOME, ERR, 0)
    np.save(tmp_path / "reads.npy", reads)
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    base = {v: os.environ[v] for v in os.environ if v != "KATOME_SORT_NODES"}

    def run(name, extra):
        out = subprocess.run([sys.executable, str(script), root, str(k), "1" if rc else "0", str(N_READS), str(READ_LEN), str(tmp_path / "reads.npy"),
                              str(tmp_path / name)], env=dict(base, **extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(tmp_path / name)

    by_edges = run("by_edges.npz", {})
    by_nodes = run("by_nodes.npz", {"KATOME_SORT_NODES": "1"})
    assert int(by_edges["n_edges"]) > 4 * 256                                               # several blocks of edges
    assert len(np.unique(by_edges["edge_src"])) < int(by_edges["n_nodes"])                  # nodes without out-edges
    assert (int(by_nodes["n_nodes"]), int(by_nodes["n_edges"])) == (int(by_edges["n_nodes"]), int(by_edges["n_edges"]))
    for a in ARRAYS:
        assert by_nodes[a].dtype == by_edges[a].dtype and by_nodes[a].tobytes() == by_edges[a].tobytes(), a
    ref = oracle.build_ascii(reads, k, rc)
    for got in (by_edges, by_nodes):
        g = types.SimpleNamespace(n_nodes=int(got["n_nodes"]), n_edges=int(got["n_edges"]), edge_label=got["edge_label"],
                                  edge_weight=got["edge_weight"].view(np.uint32), edge_src=got["edge_src"].view(np.uint64),
                                  edge_dst=got["edge_dst"].view(np.uint64))
        _assert_same_as_reference_order(g, ref)
