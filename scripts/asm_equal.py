"""Build container: is the DEVICE code of csrc/gclm_pass.hip at git revision REV, instruction for instruction, the code of the
working tree?  (Round 6 pruned the closed A/B switches from the hot file; identical device assembly means identical bits and
identical speed by construction -- stronger than the ISA statistics and than any measured A/B.)

usage: python scripts/asm_equal.py [-v] [--rename REGEX=REPLACEMENT ...] REV [FILE=gclm_pass.hip ...] [-- FILE ...]
The files before `--` are taken at REV, those after it from the working tree (none: the same names), so code that moved
between files is followed: `asm_equal.py REV gclm_update.hip -- gclm_update.hip gclm_fields.hip gclm_synth.hip`.  Several
files are always compared symbol by symbol over the union of their symbols, and the report names every symbol that differs
or exists on one side only (-v: with the first lines of its diff); exit status 0 when there is none.
--rename (any number): re.sub(REGEX, REPLACEMENT) on every assembly line of REV before the comparison, for a kernel whose
symbol changed (a new template argument, a new trailing kernel argument) and whose code should not have.
Compiles each file of both trees with the Makefile's flags to gfx950 assembly (-S --cuda-device-only), drops comments, debug /
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


def assembly(tree, name, renames=()):
    out = tempfile.mktemp(suffix=".s")
    flags = FLAGS + (PASS if name == "gclm_pass.hip" else [])
    subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-o", out, os.path.join(tree, "geocalib_amd", "csrc", name)], check=True,
                   capture_output=True)
    lines = []
    for ln in open(out):
        for pattern, replacement in renames:
            ln = re.sub(pattern, replacement, ln)
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
        elif re.match(r"\s*\.section\s+\.AMDGPU\.gpr_maximums", ln) and not key.startswith("<tail"):
            own = []                               # the padding behind the last function belongs to the file, not to it
            while out[key] and re.match(r"\s*\.(text|p2alignl|fill)\b", out[key][-1]):
                own.insert(0, out[key].pop())
            key = "<tail>"
            out[key] = own
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


def union(tree, names, renames=()):
    """({symbol: lines} over the files, {file-level block: lines}, assembly lines, kernels, source lines) of `names` in `tree`."""
    syms, per_file, n_asm, kernels, n_src = {}, {}, 0, 0, 0
    for name in names:
        lines = assembly(tree, name, renames)
        n_asm += len(lines)
        kernels += sum(1 for ln in lines if ln.strip().startswith(".amdhsa_kernel"))
        n_src += sum(1 for _ in open(os.path.join(tree, "geocalib_amd", "csrc", name)))
        bl = blocks(lines)
        assert sum(map(len, bl.values())) == len(lines)
        for k, v in bl.items():
            if k.startswith("<"):
                per_file[f"{k} of {name}"] = v
            else:
                assert k not in syms, (k, name)        # one definition per symbol over the set
                syms[k] = v
    return syms, per_file, n_asm, kernels, n_src


def main():
    args = sys.argv[1:]
    verbose = "-v" in args
    args = [x for x in args if x != "-v"]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    rev, rest = args[0], args[1:]
    old_names = rest[:rest.index("--")] if "--" in rest else rest
    old_names = old_names or ["gclm_pass.hip"]
    new_names = rest[rest.index("--") + 1:] if "--" in rest else old_names
    with tempfile.TemporaryDirectory() as old:
        for path in ("geocalib_amd/csrc", "include"):
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, path], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        sa, fa, asm_a, kernels, src_a = union(old, old_names, renames)
    sb, fb, asm_b, _, src_b = union(ROOT, new_names)
    if old_names == new_names:                     # the same files: their heads and tails must agree as well
        sa.update(fa)
        sb.update(fb)
    only = sorted(set(sa) ^ set(sb))
    differ = [k for k in sa if k in sb and sa[k] != sb[k]]
    same = not only and not differ
    print(f"{' '.join(old_names)} at {rev} ({src_a} source lines) vs {' '.join(new_names)} in the working tree ({src_b} source "
          f"lines): {asm_a} / {asm_b} assembly lines, {kernels} kernels, {len(sa)} / {len(sb)} blocks compared by name: "
          f"{'IDENTICAL' if same else f'{len(sa) - len(differ) - sum(k in sa for k in only)} IDENTICAL, {len(differ)} DIFFERENT'}")
    for pattern, replacement in renames:           # (a report says what it compared: its renames can be given again as printed)
        print(f"    --rename '{pattern}={replacement}'")
    for k in only:
        print("    only in", rev if k in sa else "the working tree", ":", k)
    import difflib
    for k in differ:
        diff = [ln for ln in difflib.unified_diff(sa[k], sb[k], lineterm="", n=0) if not ln.startswith(("---", "+++", "@@"))]
        print(f"    DIFFERENT {k}: {len(sa[k])} -> {len(sb[k])} lines, -{sum(ln[0] == '-' for ln in diff)} +{sum(ln[0] == '+' for ln in diff)}")
        for ln in diff[:40] if verbose else []:
            print("       ", ln)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
