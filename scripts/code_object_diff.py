"""Per-symbol comparison of the gfx950 code in two builds of librt_hip.so (the recipe of DESIGN.md section 4, "Ray queries").

    python scripts/code_object_diff.py OLD.so NEW.so [--llvm-bin DIR]

Takes the .hip_fatbin section of each library apart into its offload bundles, unbundles the gfx950 code object of each, disassembles it
and compares the instruction stream of every symbol of OLD with the symbol of the same name in NEW, addresses dropped.  Prints the
symbols of OLD that differ or are missing, the counts, and the symbols only NEW has; exits 1 when a symbol of OLD differs."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile


def symbols(lib, llvm, work):
    os.makedirs(work, exist_ok=True)
    raw = os.path.join(work, "fatbin")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, raw])
    data = open(raw, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
    out = collections.defaultdict(list)
    for i, at in enumerate(starts):
        bundle, code = os.path.join(work, f"bundle{i}"), os.path.join(work, f"code{i}")
        with open(bundle, "wb") as f:
            f.write(data[at:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={bundle}", f"--output={code}"])
        current = None
        for line in subprocess.check_output([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", code]).decode().splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                current = m.group(1)
                out[current].append([])
            elif current and line.strip():
                out[current][-1].append(re.sub(r"^[0-9a-f]+:\s*", "", re.sub(r"//.*$", "", line).strip()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--llvm-bin", default="/opt/rocm/lib/llvm/bin")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = symbols(args.old, args.llvm_bin, os.path.join(tmp, "old")), symbols(args.new, args.llvm_bin, os.path.join(tmp, "new"))
    same = instructions = different = 0
    for name, bodies in a.items():  # a name can occur in several code objects (inline functions of a shared header)
        if name in b and sorted(map(tuple, bodies)) == sorted(map(tuple, b[name])):
            same += len(bodies)
            instructions += sum(len(x) for x in bodies)
        else:
            different += 1
            print("differs or is missing:", name)
    print(f"old: {sum(len(v) for v in a.values())} symbols, {len(a)} distinct names; identical {same} ({instructions} instructions); different {different}")
    print("only in new:", sorted(k for k in b if k not in a))
    sys.exit(1 if different else 0)


if __name__ == "__main__":
    main()
