"""sha256 of the .text / .rodata sections of the gfx950 code object inside one or more builds of libnmpc_hip.so.

    python tools/code_object_hash.py [--renamed 'PATTERN=REPLACEMENT' ...] [lib.so ...]          (default: the in-tree library)

Two builds whose hashes agree run the same device code: the check behind "moved out of the product headers without
changing a single instruction" (profiles/r06_hygiene_code_object_identity.txt) and behind any A/B claim of "same bits".
Host-side changes (layout bookkeeping, the C ABI) do not show up here by construction. Where .text agrees and .rodata does not,
the kernel descriptors in .rodata are compared field by field: renamed kernels change the sizes of the name tables in front of
.rodata, and with them the distance from a descriptor to its code, which the descriptor records. A kernel that one build has under another
name is compared too where ``--renamed`` says so: PATTERN is a regular expression on the demangled names of the first build,
REPLACEMENT (``re.sub`` syntax) gives the name in the second.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
DEFAULT_LIB = os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "libnmpc_hip.so")


def code_object_hashes(lib):
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "gfx950.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True,
                       capture_output=True)
        out = {}
        for sec in (".text", ".rodata"):
            raw = os.path.join(td, sec.strip(".") + ".bin")
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", f"--only-section={sec}", co, raw], check=True)
            data = open(raw, "rb").read()
            out[sec] = (len(data), hashlib.sha256(data).hexdigest())
            out[sec + " bytes"] = data
        # per kernel: the bytes of each function symbol of .text (a kernel whose instructions did not change keeps its hash
        # even when a neighbour grew or shrank; branch offsets inside a function are relative)
        text = open(os.path.join(td, "text.bin"), "rb").read()
        base = None
        for line in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", co], check=True, capture_output=True,
                                   text=True).stdout.splitlines():
            m = re.search(r"\]\s+(\.text|\.rodata)\s+PROGBITS\s+([0-9a-f]+)", line)
            if m:
                out[m.group(1) + " address"] = int(m.group(2), 16)
        base = out.get(".text address")
        kernels = {}
        for line in subprocess.run(["nm", "-S", co], check=True, capture_output=True, text=True).stdout.splitlines():
            m = re.match(r"([0-9a-f]+) ([0-9a-f]+) [Tt] (\S+)$", line)
            if m and not m.group(3).endswith(".kd") and base is not None:
                a, n = int(m.group(1), 16) - base, int(m.group(2), 16)
                kernels[m.group(3)] = (n, hashlib.sha256(text[a:a + n]).hexdigest())
        out["kernels"] = kernels
    return out


def demangle(names):
    try:
        return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.strip().split("\n")
    except (OSError, subprocess.CalledProcessError):
        return list(names)


if __name__ == "__main__":
    args, renamed = sys.argv[1:], []
    while "--renamed" in args:
        k = args.index("--renamed")
        renamed.append(args[k + 1].split("=", 1))
        del args[k:k + 2]
    libs = args or [DEFAULT_LIB]
    seen = []
    for lib in libs:
        h = code_object_hashes(lib)
        seen.append(h)
        print(lib)
        for sec in (".text", ".rodata"):
            n, digest = h[sec]
            print(f"  {sec:8s} {n:9d} B  sha256 {digest}")
        print(f"  {len(h['kernels'])} kernels")
    if len(seen) == 2:
        a, b = seen[0]["kernels"], seen[1]["kernels"]
        same = sorted(k for k in a if k in b and a[k] == b[k])
        diff = sorted(k for k in a if k in b and a[k] != b[k])
        only = sorted(set(a) ^ set(b))
        print(f"kernels byte-identical: {len(same)} of {len(set(a) | set(b))}")
        new_name = dict(zip(demangle(sorted(b)), sorted(b)))
        for k, d in zip(list(only), demangle(only)):                       # renamed kernels: compared under both names
            to = [re.sub(pat, rep, d) for pat, rep in renamed if k in a and re.search(pat, d)]
            if to and new_name.get(to[0]) in only:
                k2 = new_name[to[0]]
                verdict = "byte-identical" if a[k] == b[k2] else f"differs ({a[k][0]} B -> {b[k2][0]} B)"
                print(f"  renamed, {verdict}: {d} -> {to[0]}  ({a[k][0]} B, sha256 {a[k][1][:16]} / {b[k2][1][:16]})")
                only.remove(k), only.remove(k2)
        for k, d in zip(diff, demangle(diff)):
            print(f"  differs: {d}  ({a[k][0]} B -> {b[k][0]} B)")
        for k, d in zip(only, demangle(only)):
            print(f"  only in one build: {d}")
        whole = seen[0][".text"] == seen[1][".text"] and seen[0][".rodata"] == seen[1][".rodata"]
        if not whole and seen[0][".text"] == seen[1][".text"]:
            # .rodata holds one 64-byte descriptor per kernel, in the order of .text; bytes 16 .. 23 are the offset from the
            # descriptor to the kernel's code, which follows from where the linker put the two sections (longer names move them)
            ra, rb = seen[0][".rodata bytes"], seen[1][".rodata bytes"]
            gap = [h[".text address"] - h[".rodata address"] for h in seen]
            rest = len(ra) == len(rb) and all(ra[i:i + 16] == rb[i:i + 16] and ra[i + 24:i + 64] == rb[i + 24:i + 64] for i in range(0, len(ra), 64))
            moved = {int.from_bytes(rb[i + 16:i + 24], "little") - int.from_bytes(ra[i + 16:i + 24], "little") for i in range(0, min(len(ra), len(rb)), 64)}
            if rest and moved == {gap[1] - gap[0]}:
                print(f"  .rodata: {len(ra) // 64} kernel descriptors, each identical apart from its offset to the code, {gap[1] - gap[0]:+d} B in all "
                      f"of them: the distance from .rodata to .text changed by as much (section layout; no instruction, no kernel setting)")
                print("IDENTICAL instructions; .rodata differs by section layout only")
                sys.exit(1)
        print("IDENTICAL device code" if whole else "device code differs in the kernels listed above")
        sys.exit(0 if whole else 1)
