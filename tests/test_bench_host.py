"""bench.py's host-side bookkeeping (no GPU): the PMC traffic behind `roofline.traffic` is only used when it was taken on
the very kernels that run now and on the same configuration."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_stale_pmc_counters_are_refused(tmp_path, monkeypatch):
    import bench
    cfg = {"reads": 1000, "read_len": 150, "k": 31, "batch_reads": 64, "tile_span": 30}
    sid = bench.source_id()
    assert len(sid) == 16 and sid == bench.source_id()                 # a function of the sources alone
    kernels = {"void some_kernel<1>": {"dispatches": 3, "fetch_kib": 10.0, "write_kib": 20.0}}
    f = tmp_path / "pmc.json"
    monkeypatch.setattr(bench, "PMC_FILE", str(f))
    parts = [("void some_kernel<1>", 2, True)]
    f.write_text(json.dumps({"config": cfg, "source_id": sid, "kernels": kernels}))
    t = bench.pmc_traffic(parts, cfg)
    assert t and t["bytes_per_launch"] == 2 * (10.0 * 2 + 20.0) * 1024            # FETCH_SIZE doubled for a streaming kernel
    f.write_text(json.dumps({"config": cfg, "source_id": "0" * 16, "kernels": kernels}))
    assert bench.pmc_traffic(parts, cfg) is None                                   # counters of other kernels
    f.write_text(json.dumps({"config": cfg, "kernels": kernels}))
    assert bench.pmc_traffic(parts, cfg) is None                                   # no id at all (round 2's file)
    f.write_text(json.dumps({"config": dict(cfg, reads=2000), "source_id": sid, "kernels": kernels}))
    assert bench.pmc_traffic(parts, cfg) is None                                   # another workload
    f.write_text(json.dumps({"config": cfg, "source_id": sid, "kernels": {}}))
    assert bench.pmc_traffic(parts, cfg) is None                                   # the kernel was not profiled


def test_committed_pmc_file_names_its_sources():
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
    assert len(d.get("source_id", "")) == 16 and d["config"]["reads"] == 200_000_000


def _fake_graph(rng, n_edges, n_nodes, key_words, label_stride, age=False):
    """a device.DeviceGraph stand-in on host tensors: u64 words in int64 views, u32 weights in int32 views"""
    import types
    import numpy as np
    import torch

    def u64(*shape):
        return torch.from_numpy(rng.integers(0, 2 ** 64, size=shape, dtype=np.uint64, endpoint=False).view(np.int64))
    return types.SimpleNamespace(
        n_edges=n_edges, n_nodes=n_nodes, key_words=key_words, label_stride=label_stride,
        edge_key=u64(n_edges, key_words), node_key=u64(n_nodes, key_words),
        edge_weight=torch.from_numpy(rng.integers(1, 2 ** 32, size=n_edges, dtype=np.uint32).view(np.int32)),
        edge_src=torch.from_numpy(rng.integers(0, 2 ** 40, size=n_edges, dtype=np.int64)),
        edge_dst=torch.from_numpy(rng.integers(0, 2 ** 40, size=n_edges, dtype=np.int64)),
        edge_label=torch.from_numpy(rng.integers(0, 256, size=(n_edges, label_stride), dtype=np.uint8)),
        edge_age=torch.from_numpy(rng.integers(0, 2 ** 31, size=n_edges, dtype=np.int32)) if age else None)


def test_dump_outputs_are_exact_floats_of_fixed_rows_within_the_limit(tmp_path):
    """--dump-outputs: float64 / float32 files only; u64 keys, ids and u32 weights come back exactly; a small graph whole; a
    large one as the same seeded rows on every call, under the byte limit"""
    import numpy as np
    import bench
    rng = np.random.default_rng(7)
    small = _fake_graph(rng, 300, 200, 1, 9)
    shapes = bench.dump_outputs(small, str(tmp_path / "small"))
    d = {n: np.load(str(tmp_path / "small" / (n + ".npy"))) for n in shapes}
    assert sorted(d) == ["edge_dst", "edge_index", "edge_key", "edge_label", "edge_src", "edge_weight", "graph_totals",
                         "node_index", "node_key"]
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert np.array_equal(d["edge_index"], np.arange(300)) and np.array_equal(d["node_index"], np.arange(200))
    keys = small.edge_key.numpy().view(np.uint64)
    hi, lo = d["edge_key"][:, 0].astype(np.uint64), d["edge_key"][:, 1].astype(np.uint64)
    assert np.array_equal((hi << np.uint64(32)) | lo, keys[:, 0])
    assert np.array_equal(d["edge_weight"].astype(np.uint64), small.edge_weight.numpy().view(np.uint32))
    assert np.array_equal(d["edge_src"].astype(np.int64), small.edge_src.numpy())
    assert np.array_equal(d["edge_label"].astype(np.uint8), small.edge_label.numpy())
    w = small.edge_weight.numpy().view(np.uint32).astype(np.int64)
    assert d["graph_totals"].tolist() == [300, 200, float(w.sum()), float(w.max())]

    limit = 256 << 10
    big = _fake_graph(rng, 20000, 30000, 2, 17, age=True)
    for out in ("a", "b"):
        bench.dump_outputs(big, str(tmp_path / out), limit=limit)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert "edge_age.npy" in names and names == sorted(os.listdir(str(tmp_path / "b")))
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in names) <= limit
    for n in names:
        assert open(str(tmp_path / "a" / n), "rb").read() == open(str(tmp_path / "b" / n), "rb").read()
    rows = np.load(str(tmp_path / "a" / "edge_index.npy")).astype(np.int64)
    assert 0 < len(rows) < 20000 and np.all(np.diff(rows) > 0)
    key = np.load(str(tmp_path / "a" / "edge_key.npy")).astype(np.uint64)
    want = big.edge_key.numpy().view(np.uint64)[rows]
    assert np.array_equal((key[:, 0::2] << np.uint64(32)) | key[:, 1::2], want)


def test_bench_refuses_steps_it_cannot_time_and_dumps_of_a_share():
    import subprocess
    for args, msg in ((["--steps", "0"], b"--steps must be >= 1"),
                      (["--gpus", "2", "--dump-outputs", "x"], b"--dump-outputs needs --gpus 1"),
                      (["--force-dist", "--dump-outputs", "x"], b"--dump-outputs needs --gpus 1")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=120)
        assert r.returncode != 0 and r.stdout.strip() == b"" and msg in r.stderr


def test_side_measurements_are_off_unless_full(monkeypatch):
    """a plain run is the headline alone: the CPU baselines and the other side measurements need --full"""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-c2"])
    a = bench.parse_args()
    assert a.full and a.no_cpu_c2 and not a.no_cpu_baseline and not a.no_extras
