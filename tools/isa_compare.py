"""Compare the gfx950 ISA of every kernel of two source trees (no GPU needed).

    python tools/isa_compare.py OLD_CSRC NEW_CSRC [render.hip observe.hip ...]

Each unit is compiled device-only to assembly with the library's flags (gym-duckietown_amd/build.py), every kernel's instruction
text is cut out (comments, directives and label numbers normalised) and the kernels of OLD are looked up in NEW by their demangled
name.  A kernel that gained trailing `bool` template parameters (a new instantiation axis defaulting to false) is matched with the
`false` instantiation of NEW.  Prints one line per OLD kernel and the NEW kernels that have no OLD counterpart; exit status 1 when a
pre-existing kernel differs."""
import os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"render.hip": ["-ffp-contract=fast"], "observe.hip": [], "physics.hip": ["-ffp-contract=off"], "dtsim_api.hip": []}


def kernels(csrc, unit, out_dir):
    s = os.path.join(out_dir, unit + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                    "-I" + csrc, "-S", "--cuda-device-only", "-o", s, os.path.join(csrc, unit)] + FLAGS[unit], check=True)
    txt = open(s).read().split("\n")
    out = {}
    for i, l in enumerate(txt):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", l)
        if not m or not any(".type\t" + m.group(1) + ",@function" in t for t in txt[max(0, i - 4):i]):
            continue
        end = next(j for j in range(i, len(txt)) if txt[j].startswith(".Lfunc_end"))
        body = []
        for t in txt[i + 1:end]:
            t = t.split(";")[0].rstrip()
            if not t.strip() or t.strip().startswith("."):
                if re.match(r"^\.LBB\d+_\d+:", t):
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t.strip()))
        filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
        name = subprocess.run([filt, m.group(1)], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
        out[re.sub(r"\(.*$", "", name)] = body
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or ["render.hip", "observe.hip"]
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        td = os.environ.get("ISA_KEEP", td)            # keep the assembly (and DIFF=<kernel> prints that kernel's unified diff)
        for unit in units:
            os.makedirs(os.path.join(td, "old"), exist_ok=True); os.makedirs(os.path.join(td, "new"), exist_ok=True)
            ko, kn = kernels(old, unit, os.path.join(td, "old")), kernels(new, unit, os.path.join(td, "new"))
            used = set()
            print(f"{unit}:")
            for name in sorted(ko):
                match = name if name in kn else None
                if match is None:                       # k<a, b> -> k<a, b, false>
                    base = name[:-1] if name.endswith(">") else name + "<"
                    sep = ", " if name.endswith(">") else ""
                    for extra in range(1, 3):
                        cand = base + sep + ", ".join(["false"] * extra) + ">"
                        if cand in kn:
                            match = cand
                            break
                if match is None:
                    print(f"   MISSING  {name}"); bad = 1
                    continue
                used.add(match)
                same = ko[name] == kn[match]
                if not same and os.environ.get("DIFF") == name:
                    import difflib
                    print("\n".join(difflib.unified_diff(ko[name], kn[match], lineterm="", n=2)))
                bad |= not same
                ren = f"  (now {match})" if match != name else ""
                print(f"   {'identical' if same else 'DIFFERS  '} {len(ko[name]):6d} lines  {name}{ren}")
            for name in sorted(set(kn) - used):
                print(f"   new      {len(kn[name]):6d} lines  {name}")
    sys.exit(bad)


if __name__ == "__main__":
    main()
