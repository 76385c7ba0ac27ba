"""Compare device assembly (hipcc --cuda-device-only -S) function by function (tooling).

  python tools/kernel_diff.py A.s [A2.s ...] -- B.s [B2.s ...]

Functions are matched by demangled name without `(anonymous namespace)::`; comments and section
directives go (a function's section follows its linkage) and local labels (.LBB<n>_) are normalised
before the text, kernel descriptor included, is compared.  Prints SAME / DIFF per function with
its instruction lines and the kernel's register, LDS and scratch figures on both sides; exits 1 on any
DIFF, on a function only one side has, or on one that several files of a side emit."""
import re
import subprocess
import sys

KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def side(paths):
    """{demangled name: [(body lines, metadata figures), one per emitting file]}"""
    out = {}
    for path in paths:
        text = open(path).read()
        meta, cur = {}, {}
        for m in re.finditer(r"^(  - |    )\.(\w+):\s*(\S*)$", text.split(".amdgpu_metadata")[1], re.M):
            cur = {} if m.group(1) == "  - " else cur
            cur[m.group(2)] = m.group(3)
            meta[cur.get("name")] = cur
        bodies = re.findall(r"^\t\.type\t(\S+),@function\n\1:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)
        names = subprocess.run(["c++filt"], input="\n".join(b[0] for b in bodies), capture_output=True, text=True, check=True).stdout.split("\n")
        for (sym, body), name in zip(bodies, names):
            lines = [re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", l.split(";")[0].replace(sym, "@").strip()) for l in body.split("\n")]
            figures = tuple(meta.get(sym, {}).get(k, "-") for k in KEYS)
            lines = [l for l in lines if l and l != ".text" and not l.startswith(".section")]   # placement follows linkage
            out.setdefault(name.replace("(anonymous namespace)::", ""), []).append((lines, figures))
    return out


def main(argv):
    a, b = side(argv[:argv.index("--")]), side(argv[argv.index("--") + 1:])
    bad = 0
    print("# verdict | instruction lines A B | " + " ".join(KEYS) + " A | B | function")
    for name in sorted(set(a) | set(b)):
        fa, fb = a.get(name, []), b.get(name, [])
        if len(fa) != 1 or len(fb) != 1:
            verdict = f"{'ONLY' if not fa or not fb else 'DUPLICATE'} A:{len(fa)} B:{len(fb)}"
        else:
            verdict = "SAME" if fa[0] == fb[0] else "DIFF"
        bad += verdict != "SAME"
        insn = [str(sum(not l.startswith(".") for l in f[0][0])) if f else "-" for f in (fa, fb)]
        print(f"{verdict} | {' '.join(insn)} | {' | '.join(' '.join(f[0][1]) if f else '-' for f in (fa, fb))} | {name}")
    print(f"# {len(a)} functions in A, {len(b)} in B, {bad} not SAME")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
