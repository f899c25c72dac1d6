"""One digest per kernel of the compiler's gfx950 assembly for a HIP translation unit: the instrument for "this refactor changed
text, not code".  Two trees whose tables agree run the same device code.

    python scripts/kernel_isa_digest.py [sage_amd/csrc/kernels.hip] [-D...]  > before.txt     (then again on the branch: after.txt)
    python scripts/kernel_isa_digest.py --compare before.txt after.txt                         (exit status 1 if a digest moved)

hipcc --cuda-device-only -S, gfx950, the flags of sage_amd/build.py.  No GPU needed.  A kernel's body is its label up to its
.Lfunc_end, which has its .amdhsa_kernel block inside.  So that a digest moves with the kernel's code and with nothing else, lines
naming the per-compilation __hip_cuid_<hash> symbol are dropped, runs of blanks collapsed, local labels lose the function's ordinal
in the file (a neighbour may leave) and the kernel's own symbol is written `@` (a renamed kernel keeps its digest).  The instances
of a library's templates (rocprim::) are one row: their count and a digest over their rows.  --library-rows prints them as rows
of their own instead (the full demangled name, insns, digest), so that their union across translation units can be compared."""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-S"]
LIBRARY = "rocprim::"


def table(src, extra=(), library_rows=False):
    run = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-x", "hip", src, "-o", "-"], capture_output=True, text=True)
    if run.returncode:
        sys.exit(run.stderr)
    lines = [ln for ln in run.stdout.split("\n") if "__hip_cuid_" not in ln]
    kernels = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    start = {ln.split(":")[0]: i for i, ln in enumerate(lines) if ln[:1] == "_" and ":" in ln}
    names = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True).stdout.split("\n")
    rows, library = [], []
    for name, dem in zip(kernels, names):
        body = lines[start[name]:]
        body = body[:next(i for i, ln in enumerate(body) if ln.startswith(".Lfunc_end")) + 1]
        body = [re.sub(r"(\.LBB|\bBB|\.LJTI|\.LCPI|\.Lfunc_end|\.Lfunc_begin)\d+", r"\1", " ".join(ln.replace(name, "@").split())) for ln in body]
        # an instruction line: not blank, not a label, a directive or a comment
        insns = sum(1 for ln in body if ln and not re.match(r"([.;]|\S+: ?(;.*)?$)", ln))
        dem = dem.replace("sagehip::(anonymous namespace)::", "").replace("sagehip::", "").replace("void ", "")
        if not (library_rows and dem.startswith(LIBRARY)):
            dem = re.sub(r"\((?!anonymous).*$", "", dem)
        row = (dem, insns, hashlib.sha256("\n".join(body).encode()).hexdigest())
        (library if dem.startswith(LIBRARY) else rows).append(row)
    if library_rows:
        return rows + sorted(library)
    if library:
        rows.append((f"{LIBRARY}* ({len(library)} instances)", sum(r[1] for r in library),
                     hashlib.sha256("\n".join(f"{r[0]} {r[2]}" for r in library).encode()).hexdigest()))
    return rows


def compare(before, after):
    def read(path):
        with open(path) as fh:
            return dict((ln.rsplit(None, 2)[0], ln.split()[-1]) for ln in fh.read().split("\n")[2:] if ln.strip())  # (a name may pass column 72)
    a, b = read(before), read(after)
    moved = [k for k in a if k in b and a[k] != b[k]]
    print(f"{len(a)} rows before, {len(b)} after, {sum(k in b for k in a)} in both, {len(moved)} of those with another digest")
    for k in moved:
        print(f"moved        {k}")
    for k, v in list(a.items()) + list(b.items()):
        if (k in a) != (k in b):
            other = [n for n, d in (b if k in a else a).items() if d == v and (n in a) != (n in b)]
            print(f"{'only before' if k in a else 'only after '}  {k}" + (f"   (same digest as {other[0]})" if other else ""))
    return 1 if moved else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(compare(args[1], args[2]))
    src = next((a for a in args if not a.startswith("-")), os.path.join(ROOT, "sage_amd", "csrc", "kernels.hip"))
    library_rows = "--library-rows" in args
    extra = [a for a in args if a.startswith("-") and a != "--library-rows"]
    print(f"# hipcc {' '.join(FLAGS + extra)} {os.path.relpath(src, ROOT)}")
    print(f"{'kernel':<72} {'insns':>7}  sha256")
    for r in table(src, extra, library_rows):
        print(f"{r[0]:<72} {r[1]:>7}  {r[2]}")
