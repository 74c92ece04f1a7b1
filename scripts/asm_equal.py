"""Build container: is the DEVICE code of csrc/gclm_pass.hip at git revision REV, instruction for instruction, the code of the
working tree?  (Round 6 pruned the closed A/B switches from the hot file; identical device assembly means identical bits and
identical speed by construction -- stronger than the ISA statistics and than any measured A/B.)

usage: python scripts/asm_equal.py REV [FILE=gclm_pass.hip]
Compiles FILE of both trees with the Makefile's flags to gfx950 assembly (-S --cuda-device-only), drops comments, debug /
file directives and the compilation-unit id symbol (a hash of the source text), and compares the rest line by line.
Where the two trees emit the same kernels in another order (the host's dispatcher decides the order of instantiation), the
comparison is made symbol by symbol: every line of the file belongs to the block of one symbol (its code, its resource
symbols, its kernel descriptor, its metadata entry) or to the file's head and tail, the two sets of symbols must be equal
and so must every line of every block.  Only the function's running number inside its local labels (.LBB<n>_<k>,
.Lfunc_end<n>) is dropped, which is the emission order itself."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast-honor-pragmas", "-S", "--cuda-device-only"]
PASS = ["-fno-slp-vectorize", "-mllvm", "-disable-vector-combine"]


def assembly(tree, name):
    out = tempfile.mktemp(suffix=".s")
    flags = FLAGS + (PASS if name == "gclm_pass.hip" else [])
    subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-o", out, os.path.join(tree, "geocalib_amd", "csrc", name)], check=True,
                   capture_output=True)
    lines = []
    for ln in open(out):
        directive = ln.lstrip().startswith(".") and not re.match(r"\.L\w+:", ln)      # (a local label's comment names its loop)
        ln = ln.rstrip() if directive else ln.split(";")[0].rstrip()
        if not ln.strip() or re.match(r"\s*\.(file|loc|ident|cfi|section\s+\.debug)", ln) or "__hip_cuid_" in ln:
            continue
        lines.append(ln)
    os.unlink(out)
    return lines


def blocks(lines):
    """{symbol: its lines} of one assembly text, plus the blocks '<head>', '<tail>' and '<metadata tail>'."""
    out, key, meta = {"<head>": []}, "<head>", False
    for i, ln in enumerate(lines):
        m = re.search(r"; -- Begin function (\S+)", ln)
        if m:                                      # a function begins; the .section / .text line before it is its own
            own = [out[key].pop()] if out[key] and re.match(r"\s*\.(section|text)", out[key][-1]) else []
            key = m.group(1)
            assert key not in out, key
            out[key] = own
        elif re.match(r"\s*\.set amdgpu\.", ln) and not key.startswith("<tail"):
            key = "<tail>"
            out[key] = []
        elif ln.startswith("amdhsa.kernels:"):
            meta = True
        elif meta and ln.startswith("  - "):       # one kernel's metadata entry: named by its .name line further down
            name = next(re.match(r"\s*\.name:\s*(\S+)", x).group(1) for x in lines[i:] if re.match(r"\s*\.name:\s*_Z", x))
            key = "metadata of " + name
            assert key not in out, key
            out[key] = []
        elif meta and ln.startswith("amdhsa."):
            key, meta = "<metadata tail>", False
            out[key] = []
        out[key].append(re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", re.sub(r"\.LBB\d+_", ".LBB_", ln)))
    return out


def main():
    rev = sys.argv[1]
    name = sys.argv[2] if len(sys.argv) > 2 else "gclm_pass.hip"
    with tempfile.TemporaryDirectory() as old:
        for path in ("geocalib_amd/csrc", "include"):
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, path], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        a, b = assembly(old, name), assembly(ROOT, name)
        n_old = sum(1 for _ in open(os.path.join(old, "geocalib_amd", "csrc", name)))
    n_new = sum(1 for _ in open(os.path.join(ROOT, "geocalib_amd", "csrc", name)))
    kernels = sum(1 for ln in a if ln.strip().startswith(".amdhsa_kernel"))
    same, how, da, db = a == b, "", a, b
    if not same:                                   # the same kernels in another order?  compare symbol by symbol
        ba, bb = blocks(a), blocks(b)
        assert sum(map(len, ba.values())) == len(a) and sum(map(len, bb.values())) == len(b)
        only = sorted(set(ba) ^ set(bb))
        differ = [k for k in ba if k in bb and ba[k] != bb[k]]
        same, how = not only and not differ, f" per symbol ({len(ba)} blocks, compared by name)"
        for k in only:
            print("    only in", rev if k in ba else "the working tree", ":", k)
        da, db = [ln for k in differ for ln in ba[k]], [ln for k in differ for ln in bb[k]]
    print(f"{name}: {rev} ({n_old} source lines) vs working tree ({n_new} source lines): {len(a)} / {len(b)} assembly lines, "
          f"{kernels} kernels, {'IDENTICAL' if same else 'DIFFERENT'}{how}")
    if not same:
        import difflib
        for ln in list(difflib.unified_diff(da, db, lineterm="", n=0))[:40]:
            print("   ", ln)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
