"""Phase clocks of the in-LDS key ordering (lds_order.h) in its two kernels, from an experiment build of the library:
    make -C katome_amd/csrc B=build_phases OUT=../../build_variants/libkatome_gpu_phases.so EXTRA=-DKATOME_LC_PHASES
    KATOME_LIB=build_variants/libkatome_gpu_phases.so python tools/lds_order_phases.py [workload] [builds]
One JSON line: shader clocks that thread 0 of every workgroup saw go by, added up over the workgroups and divided by the builds.
A stamped build is for this split only; kernel times come from the shipped library."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401
from katome_amd import device as kd  # noqa: E402
from katome_amd._lib import lib  # noqa: E402
from katome_amd.workloads import WORKLOADS  # noqa: E402

LO = ["read_out_and_kept", "count", "scan", "place", "rank", "write"]
GM = ["load_b", "count", "scan", "place", "rank", "write", "merge_steps"]


def read(name, n):
    f = getattr(lib(), name)
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * n)()
    if f(out):
        raise RuntimeError(name)
    return list(out)


def main():
    wl = WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "c3"]
    builds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    packed, _ = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, 0)
    batch = 16 << 20
    for it in range(builds + 1):                 # (the first build is not counted)
        b = kd.Builder(wl.k, True, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2))
        for r0 in range(0, wl.reads, batch):
            b.count_reads(packed, min(batch, wl.reads - r0), wl.read_len, None, first_read=r0)
        dg = b.finalize()
        n_edges = dg.n_edges
        del dg
        b.close()
        if it == 0:
            read("katome_debug_lc_phases", 16), read("katome_debug_lo_phases", 8), read("katome_debug_gm_phases", 8)
    lc, lo, gm = read("katome_debug_lc_phases", 16), read("katome_debug_lo_phases", 8), read("katome_debug_gm_phases", 8)
    print(json.dumps({"workload": wl.name, "builds": builds, "n_edges": n_edges,
                      "lds_count_ordered_kernel": {"clear": lc[12] // builds, "insert": lc[13] // builds, "read_out_and_order": lc[14] // builds,
                                                   "write": lc[15] // builds,
                                                   "regions": {n: lc[4 + i] // builds for i, n in enumerate(("s1_and_registers", "digit_count", "scan_and_reserve", "reorder"))},
                                                   "order": {n: lo[i] // builds for i, n in enumerate(LO)}},
                      "group_merge_kernel": {n: gm[i] // builds for i, n in enumerate(GM)}}))


if __name__ == "__main__":
    main()
