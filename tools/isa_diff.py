"""Compare two device assembly listings kernel by kernel (a refactor's "the compiler's output did not move").

Build both listings on the CPU, e.g. of the parent commit and of the working tree:
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude --cuda-device-only -S \
      llmvox_amd/csrc/ar_kernels.hip -o /tmp/new.s
then
  python tools/isa_diff.py /tmp/old.s /tmp/new.s [--rename REGEX=REPL ...] [--show N]
pairs the kernels by mangled name and compares each one's instruction stream: the lines between the
kernel's label and its .Lfunc_end, comments and assembler directives dropped, the function number in
local labels (.LBB<n>_) dropped. It prints which kernels are identical, which differ and by how many
diff lines, and for those that differ the resource figures of both sides from the listing's
"; Kernel info:" block (SGPRs, VGPRs, AGPRs, scratch and LDS bytes, occupancy).
--rename rewrites names of the OLD listing before pairing (re.sub), for a kernel whose template
arguments changed, e.g. a dropped `Li2E`:
  --rename 'ar_attn_v2_kernelI(\\w+?)Li2E=ar_attn_v2_kernelI\\1'
--show N prints the first N diff lines of each kernel that differs.
Exit status 0 when every kernel is identical, 1 otherwise. It only compares: no instruction is searched for."""
import difflib
import re
import sys

FIGS = ["TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy"]


def parse(path, renames):
    """{mangled name: (instruction lines, {figure: value})} of a listing, in file order"""
    def ren(s):
        for pat, repl in renames:
            s = re.sub(pat, repl, s)
        return s

    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        name = ren(m.group(1))
        body = []
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            t = lines[i].split(";")[0].strip()
            i += 1
            if not t:
                continue
            if t.startswith("."):
                if not re.match(r"^\.LBB\d+_\d+:$", t):
                    continue  # a directive (the .amdhsa_kernel block sits ahead of .Lfunc_end)
            body.append(ren(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(t.split()))))
        figs = {}
        while i < len(lines) and not lines[i].startswith("; Kernel info:"):
            if re.match(r"^_Z\w+:", lines[i]):
                break  # a device function: no kernel info
            i += 1
        else:
            i += 1
            while i < len(lines) and lines[i].startswith(";"):
                f = re.match(r"^; (\w+): (\d+)", lines[i])
                if f and f.group(1) in FIGS:
                    figs[f.group(1)] = int(f.group(2))
                i += 1
        out[name] = (body, figs)
    return out


def main(argv):
    renames, show, paths = [], 0, []
    it = iter(argv)
    for a in it:
        if a == "--rename":
            pat, repl = next(it).split("=", 1)
            renames.append((pat, repl))
        elif a == "--show":
            show = int(next(it))
        else:
            paths.append(a)
    if len(paths) != 2:
        sys.exit(__doc__)
    old, new = parse(paths[0], renames), parse(paths[1], [])
    same, moved = [], []
    for name, (body, figs) in new.items():
        if name not in old:
            continue
        if old[name][0] == body:
            same.append(name)
        else:
            d = [x for x in difflib.unified_diff(old[name][0], body, lineterm="", n=0)
                 if x[:1] in "+-" and x[:3] not in ("+++", "---")]
            moved.append((name, d))
    print(f"kernels: {len(old)} old, {len(new)} new, {len(same) + len(moved)} paired by name")
    print(f"identical: {len(same)}")
    for name in same:
        print(f"  = {name}")
    print(f"different: {len(moved)}")
    for name, d in moved:
        o, n = old[name], new[name]
        print(f"  ! {name}")
        print(f"      instructions {len(o[0])} -> {len(n[0])}, {len(d)} diff lines")
        print("      old " + " ".join(f"{k}={o[1].get(k)}" for k in FIGS))
        print("      new " + " ".join(f"{k}={n[1].get(k)}" for k in FIGS))
        print("      resources " + ("equal" if o[1] == n[1] else "DIFFER"))
        for x in d[:show]:
            print("        " + x)
    for name in old:
        if name not in new:
            print(f"only in old: {name}")
    for name in new:
        if name not in old:
            print(f"only in new: {name}")
    return 0 if not moved and len(same) == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
