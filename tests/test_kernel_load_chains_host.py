"""tools/kernel_load_chains.py on short hand-written listings: the L / W / w / B string of a function and its longest chain of
`one to three loads, then vmcnt(0)`.  No GPU and no library: the parser takes assembly text."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_load_chains", os.path.join(ROOT, "tools", "kernel_load_chains.py"))
klc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(klc)

_SERIAL = "\n".join("""\tglobal_load_dwordx4 v[%d:%d], v[2:3], off nt
\ts_waitcnt vmcnt(0)
\tv_mul_lo_u32 v40, v%d, s4""" % (8 + 4 * j, 11 + 4 * j, 8 + 4 * j) for j in range(8))

_LISTING = """
lib.co:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001000 <serial_kernel>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                          // 000000001000: C0060002 00000000
\ts_waitcnt lgkmcnt(0)
\ts_barrier
%s
\ts_barrier
\ts_endpgm

0000000000002000 <paired_kernel>:
\tglobal_load_dwordx2 v[4:5], v[0:1], off
\tglobal_load_dword v6, v[2:3], off
\ts_waitcnt vmcnt(1)
\tv_add_u32 v7, v4, v5
\tglobal_load_dwordx2 v[8:9], v[0:1], off offset:2048
\tglobal_load_dword v10, v[2:3], off offset:1024
\ts_waitcnt vmcnt(2) lgkmcnt(0)
\tv_add_u32 v7, v7, v6
\ts_endpgm

0000000000003000 <no_loads_kernel>:
\tv_mov_b32 v1, 0
\tds_write_b32 v0, v1
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v[2:3], v1, off
\ts_endpgm
""" % _SERIAL


def test_the_strings_of_a_listing():
    s = klc.load_strings(_LISTING)
    assert list(s) == ["serial_kernel", "paired_kernel", "no_loads_kernel"]
    assert s["serial_kernel"] == "B" + "LW" * 8 + "B"          # (lgkmcnt alone is no wait for a load; the scalar load is no L)
    assert s["paired_kernel"] == "LLwLLw"
    assert s["no_loads_kernel"] == ""


def test_a_chain_of_eight():
    assert klc.longest_chain(klc.load_strings(_LISTING)["serial_kernel"]) == 8


def test_partial_waits_make_no_chain():
    assert klc.longest_chain("LLwLLw") == 0


def test_no_loads_no_chain():
    assert klc.longest_chain("") == 0 and klc.longest_chain("BWB") == 0


def test_what_ends_and_what_joins_a_chain():
    assert klc.longest_chain("LLwWLLwWLLwW") == 3              # a partial wait inside a unit is looked through
    assert klc.longest_chain("LWWWLWWW") == 2                  # a second vmcnt(0) waits for nothing
    assert klc.longest_chain("LLLLLLLLLLWLLWLLWLLWW") == 3     # ten loads together are no unit; the three pairs behind them are
    assert klc.longest_chain("LWBLW") == 1                     # a barrier parts two chains
    assert klc.longest_chain("LLLLWLW") == 1                   # four loads and a wait: no unit
    assert klc.longest_chain("LWLWLLLLLLLLWLWLWLW") == 3       # the longest of several


def test_compact():
    assert klc.compact("BLLLLLLLLLLWLLWW") == "B L*10 W LL WW"
    assert klc.compact("") == ""
