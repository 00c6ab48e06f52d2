"""Which kernels of two builds of the library differ: every gfx950 kernel disassembled, addresses dropped, compared per symbol
(a default template argument added to a kernel changes its mangled name and nothing else: ArraySource is dropped from the names).
    python tools/kernel_isa_diff.py PARENT.so [THIS.so]"""
import os, re, struct, subprocess, sys, tempfile, hashlib
LLVM = "/opt/rocm/lib/llvm/bin"; MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
def kernels(lib):
    data = open(lib, "rb").read(); at = 0; out = {}
    while True:
        at = data.find(MAGIC, at)
        if at < 0: break
        n = struct.unpack_from("<Q", data, at + 24)[0]; p = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p); p += 24
            triple = data[p:p + tl].decode(); p += tl
            if "gfx950" not in triple: continue
            with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
                f.write(data[at + off: at + off + size]); path = f.name
            dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True).stdout
            os.unlink(path)
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m: cur = m.group(1); out.setdefault(cur, []); continue
                if cur and line.strip():
                    out[cur].append(re.sub(r"\s*//.*$", "", line).strip())
        at += len(MAGIC)
    # (the filler behind the last kernel of a section is the file's, not the kernel's: it moves when another kernel comes last)
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."): body.pop()
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.splitlines()
    res = {}
    for mangled, dem in zip(out, names):
        dem = dem.replace(" ", "").replace(",katome::ArraySource>", ">").replace("katome::ArraySource)", ")").replace(", katome::ArraySource)", ")")
        dem = re.sub(r"(lds_count_ordered_kernel<\w+),false>", r"\1>", dem)          # (REGIONS = false: the kernel as it was)
        dem = dem.replace("(anonymousnamespace)::", "")                             # (or every such kernel would be cut down to "katome::" below)
        dem = re.sub(r"\(.*$", "", dem)
        res[dem] = (len(out[mangled]), hashlib.sha1("\n".join(out[mangled]).encode()).hexdigest())
    return res
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
a = kernels(sys.argv[1]); b = kernels(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "katome_amd", "lib", "libkatome_gpu.so"))
same = [k for k in a if k in b and a[k] == b[k]]
print("kernels: parent %d, tree %d, identical %d" % (len(a), len(b), len(same)))
for k in sorted(a):
    if k not in b: print("GONE  ", k)
    elif a[k] != b[k]: print("DIFFER", k, a[k][0], "->", b[k][0])
for k in sorted(b):
    if k not in a: print("NEW   ", k, b[k][0])
