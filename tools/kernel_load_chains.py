"""How the library's kernels wait for their global loads: per gfx950 kernel whose (demangled) name holds a pattern, the order of
    L  a global_load*            W  s_waitcnt vmcnt(0)            w  s_waitcnt vmcnt(n > 0)            B  s_barrier
in the disassembly's text order, and the longest CHAIN in it: units of one to three loads and then a vmcnt(0), one behind the other
(`LWLWLW`: 3, `LLwWLLwW`: 2; partial waits in between do not break a unit, a barrier or a fourth load does).  Every unit of a chain
is a memory latency that the next unit's loads wait behind; a guarded load in an unrolled loop (`if (i < n) x[j] = p[i]`) makes one.
    python tools/kernel_load_chains.py [PATTERN [libkatome_gpu.so]]      (no pattern: every kernel)
One line per kernel, sorted by name: chain length, loads, the name, the string (a run of four and more as L*10)."""
import os, re, struct, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

_HEAD = re.compile(r"^(?:[0-9a-f]+ )?<(.+)>:$")
_VMCNT = re.compile(r"\bvmcnt\((\d+)\)")
_CHAIN = re.compile(r"(?<!L)(?:L{1,3}W)+")


def load_strings(text):
    """assembly text (llvm-objdump -d: `<name>:` heads a function) -> {name: its L / W / w / B string}"""
    out, cur = {}, None
    for line in text.splitlines():
        t = re.sub(r"\s*//.*$", "", line).strip()
        m = _HEAD.match(t)
        if m:
            cur = m.group(1); out.setdefault(cur, ""); continue
        if cur is None or not t:
            continue
        op = t.split()[0]
        if op.startswith("global_load"):
            out[cur] += "L"
        elif op == "s_barrier":
            out[cur] += "B"
        elif op == "s_waitcnt":
            m = _VMCNT.search(t)
            if m:
                out[cur] += "W" if int(m.group(1)) == 0 else "w"
    return out


def longest_chain(s):
    """units of `one to three loads, then vmcnt(0)` that follow each other without a gap; partial waits are looked through"""
    s = re.sub(r"W+", "W", s.replace("w", ""))                  # (a second vmcnt(0) waits for nothing)
    return max((m.group(0).count("W") for m in _CHAIN.finditer(s)), default=0)


def compact(s):
    """LLLLLLLLLLWLLW -> L*10 W LL W: runs of four and more as letter*count"""
    return " ".join(m.group(0) if len(m.group(0)) < 4 else "%s*%d" % (m.group(1), len(m.group(0))) for m in re.finditer(r"(.)\1*", s))


def disassembly(lib):
    """the text of every gfx950 code object in the library (as tools/kernel_regs.py finds them)"""
    data = open(lib, "rb").read(); at = 0; text = []
    while True:
        at = data.find(MAGIC, at)
        if at < 0:
            break
        n = struct.unpack_from("<Q", data, at + 24)[0]
        p = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p); p += 24
            triple = data[p:p + tl].decode(); p += tl
            if "gfx950" not in triple:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
                f.write(data[at + off: at + off + size]); path = f.name
            text.append(subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True).stdout)
            os.unlink(path)
        at += len(MAGIC)
    return "\n".join(text)


def main(argv):
    pat = argv[1] if len(argv) > 1 else ""
    lib = argv[2] if len(argv) > 2 else os.path.join(ROOT, "katome_amd", "lib", "libkatome_gpu.so")
    strings = load_strings(disassembly(lib))
    names = subprocess.run(["c++filt"], input="\n".join(strings), capture_output=True, text=True).stdout.splitlines()
    rows = []
    for mangled, dem in zip(strings, names):
        dem = re.sub(r"\)\s*(\[clone.*)?$", ")", dem.replace("(anonymous namespace)::", ""))
        dem = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", dem)          # (the argument list)
        if pat in dem:
            rows.append((dem, strings[mangled]))
    for dem, s in sorted(rows):
        print("chain %2d  loads %3d  %s  %s" % (longest_chain(s), s.count("L"), dem, compact(s) or "-"))


if __name__ == "__main__":
    main(sys.argv)
