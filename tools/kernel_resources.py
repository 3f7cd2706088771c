"""Per-kernel register / scratch / LDS use of one csrc file, from hipcc's device asm (cross-compiles, no GPU needed).

    python tools/kernel_resources.py gemm.hip [regex] [-D...]      # prints one line per kernel whose demangled-ish name matches
    python tools/kernel_resources.py attention.hip --against REV   # is every kernel's ISA the one git revision REV generates?

--against compiles the source from the working tree and from REV's csrc/ + include/ovhip.h with the same flags, cuts each kernel from
its label to s_endpgm and compares the instruction text (comments, .file / .loc / .ident and the per-compilation __hip_cuid_ symbol
dropped).  Exit status 1 if any kernel differs: identical ISA under untouched host code is the same bits at the same speed.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd import build as B  # noqa: E402

CSRC_REL = os.path.relpath(B.CSRC, ROOT)
HEADER_REL = os.path.join("include", "ovhip.h")         # common.h includes ../../include/ovhip.h


def resources(src, extra=(), csrc=None):
    out = subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-o", "-",
                          *extra, os.path.join(csrc or B.CSRC, src)], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
    res = {}
    for blk in out.split("  - .agpr_count:")[1:]:
        def g(k):
            m = re.search(r"\." + k + r":\s+(\S+)", blk)
            return m.group(1) if m else "?"
        res[g("name")] = dict(agpr=blk.split("\n")[0].strip(), vgpr=g("vgpr_count"), sgpr=g("sgpr_count"), scratch=g("private_segment_fixed_size"),
                              lds=g("group_segment_fixed_size"), spill=g("vgpr_spill_count"))
    return res, out


def kernel_bodies(asm_text):
    """Assembly text -> {kernel label: its lines up to s_endpgm}, without what changes from one compilation of the same code to the
    next: comments (whole-line and trailing; the ;;#ASMSTART / ;;#ASMEND markers go with them), blank lines, .file / .loc / .ident and
    every line that names the __hip_cuid_<hash> symbol."""
    out = {}
    for fm in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?s_endpgm)", asm_text, re.S | re.M):
        lines = []
        for line in fm.group(2).split("\n"):
            t = line.split(";")[0].strip()
            if not t or "__hip_cuid_" in t or re.match(r"\.(file|loc|ident)\b", t):
                continue
            lines.append(re.sub(r"\s+", " ", t))
        out[fm.group(1)] = lines
    return out


def differing_lines(a, b):
    """Number of positions at which two kernels' normalised line lists differ (a length difference counts line by line)."""
    return sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))


def checkout_sources(rev, dest):
    """REV's csrc/* and include/ovhip.h under dest, in the repository's relative layout; returns that csrc directory."""
    names = subprocess.run(["git", "-C", ROOT, "ls-tree", "-r", "--name-only", rev, "--", CSRC_REL, HEADER_REL], check=True,
                           stdout=subprocess.PIPE, text=True).stdout.split()
    for rel in names:
        path = os.path.join(dest, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{rel}"], check=True, stdout=subprocess.PIPE).stdout)
    return os.path.join(dest, CSRC_REL)


def compare(src, rev, pat=".", extra=()):
    """Prints one line per kernel of src; returns the number of kernels whose ISA differs from rev's (a kernel on one side only differs)."""
    with tempfile.TemporaryDirectory() as tmp:
        old_res, old_asm = resources(src, extra, checkout_sources(rev, tmp))
    new_res, new_asm = resources(src, extra)
    old, new = kernel_bodies(old_asm), kernel_bodies(new_asm)
    ndiff = 0
    for name in sorted(set(old) | set(new)):
        if not re.search(pat, name):
            continue
        n = differing_lines(old.get(name, []), new.get(name, []))
        ndiff += n != 0

        def fmt(r):
            return f"vgpr {r['vgpr']:>3} sgpr {r['sgpr']:>3} scratch {r['scratch']:>3} lds {r['lds']:>5}" if r else "absent"
        print(f"{name[:96]:<96} {'identical' if n == 0 else f'differs ({n} lines)':<20} {rev}: {fmt(old_res.get(name))} | now: {fmt(new_res.get(name))}")
    return ndiff


if __name__ == "__main__":
    args = sys.argv[1:]
    rev = None
    if "--against" in args:
        i = args.index("--against")
        rev = args[i + 1]
        del args[i:i + 2]
    src = args[0]
    pat = next((a for a in args[1:] if not a.startswith("-")), ".")
    extra = [a for a in args[1:] if a.startswith("-")]
    if rev is not None:
        sys.exit(1 if compare(src, rev, pat, extra) else 0)
    res, _ = resources(src, extra)
    for name, r in sorted(res.items()):
        if re.search(pat, name):
            print(f"{name[:110]:<110} vgpr {r['vgpr']:>3} agpr {r['agpr']:>3} sgpr {r['sgpr']:>3} scratch {r['scratch']:>4} lds {r['lds']:>6}")
