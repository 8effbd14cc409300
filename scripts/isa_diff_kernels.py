"""Do the kernels of one HIP source compile to the same gfx950 code as at another revision?

Compiles csrc/<file> as it stands and as `git show <rev>:…` gives it, both with the Makefile's flags (device only, to assembly), cuts
the assembly into kernels (.amdhsa_kernel symbols with their text and their descriptor), renames the local labels in order of
appearance and compares kernel by kernel, by demangled name.  Prints the kernels that differ, those only one side has, and a count;
exit status 1 if a kernel that both sides have differs.
      python scripts/isa_diff_kernels.py ah_group_agg.hip [--rev HEAD~1] [--only typed_]
"""
import argparse, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]


def kernels(path, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-o", out, path])
    text = open(out).read()
    names = re.findall(r"\.amdhsa_kernel (\S+)", text)
    found = {}
    for sym in names:
        body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.section\s+\.rodata.*?\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % (re.escape(sym), re.escape(sym)), text, re.S | re.M)
        assert body, sym
        code = "\n".join(l for l in (body.group(1) + body.group(2)).splitlines() if l.strip() and not l.lstrip().startswith(";"))
        code = re.sub(r"\s*;.*", "", code)   # trailing comments (encodings are not printed; offsets and notes are)
        labels = {}
        for m in re.finditer(r"\.LBB\d+_\d+|\.Ltmp\d+|\.Lfunc_\w+", code):
            labels.setdefault(m.group(0), "L%d" % len(labels))
        code = re.sub(r"\.LBB\d+_\d+|\.Ltmp\d+|\.Lfunc_\w+", lambda m: labels[m.group(0)], code)
        found[sym] = code
    dem = subprocess.run(["c++filt"] + list(found), capture_output=True, text=True).stdout.splitlines()
    return {d.replace("(anonymous namespace)::", ""): found[s] for s, d in zip(found, dem)}


ap = argparse.ArgumentParser()
ap.add_argument("file")
ap.add_argument("--rev", default="HEAD~1")
ap.add_argument("--only", default="", help="compare kernels whose name contains this only")
args = ap.parse_args()
with tempfile.TemporaryDirectory() as d:
    old_src = os.path.join(d, "old_" + args.file)
    open(old_src, "w").write(subprocess.check_output(["git", "-C", ROOT, "show", f"{args.rev}:arrow_go_amd/csrc/{args.file}"], text=True))
    new = kernels(os.path.join(CSRC, args.file), os.path.join(d, "new.s"))
    old = kernels(old_src, os.path.join(d, "old.s"))
keep = lambda ks: {k: v for k, v in ks.items() if args.only in k}   # noqa: E731
new, old = keep(new), keep(old)
both = sorted(set(new) & set(old))
differ = [k for k in both if new[k] != old[k]]
for k in differ:
    print("DIFFERS ", k[:140])
for k in sorted(set(old) - set(new)):
    print("GONE    ", k[:140])
print(f"{len(both)} kernels on both sides, {len(both) - len(differ)} identical, {len(differ)} differ, {len(set(new) - set(old))} new, {len(set(old) - set(new))} gone")
sys.exit(1 if differ else 0)
