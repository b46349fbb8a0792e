"""Compare the gfx950 ISA of every kernel of two source trees (no GPU needed).

    python tools/isa_compare.py OLD_CSRC NEW_CSRC [unit ...]        (default: every unit of gym-duckietown_amd/build.py)

Each unit is compiled device-only to assembly with the library's flags (build.py), every kernel's instruction text is cut out
(comments, directives and label numbers normalised) and the kernels of OLD are looked up by their demangled name in ALL units of NEW
(a kernel that moved is printed with its new unit).  A kernel that gained trailing `bool` template parameters (a new instantiation
axis defaulting to false) is matched with the `false` instantiation of NEW.  Prints one line per OLD kernel -- for one that differs
also whether the instruction count, the multiset of opcodes and the .amdhsa VGPR / SGPR / scratch / LDS numbers are the same -- and the
NEW kernels that have no OLD counterpart; exit status 1 when a pre-existing kernel differs."""
import collections, difflib, os, re, shutil, subprocess, sys, tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-duckietown_amd"))
import build as dtbuild

AMDHSA = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(csrc, unit, out_dir):
    """{demangled name: (instruction lines, (vgpr, sgpr, scratch, lds))} of one unit; {} where the tree has no such unit."""
    if not os.path.exists(os.path.join(csrc, unit)):
        return {}
    os.makedirs(out_dir, exist_ok=True)
    s = os.path.join(out_dir, unit + ".s")
    subprocess.run(dtbuild.compile_cmd(os.path.join(csrc, unit), s, ["-I" + csrc, "-w"], asm=True), check=True)
    whole = open(s).read(); txt = whole.split("\n")
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
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
        hsa = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", whole, re.S)
        res = tuple(int(re.search(r"\.amdhsa_" + k + r" (\d+)", hsa.group(1)).group(1)) for k in AMDHSA) if hsa else ()
        name = subprocess.run([filt, m.group(1)], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
        out[re.sub(r"\(.*$", "", name)] = (body, res)
    return out


def ops(body):
    return collections.Counter(t.split()[0] for t in body if not t.endswith(":"))

def main():
    old, new = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or list(dtbuild.UNITS)
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        td = os.environ.get("ISA_KEEP", td)            # keep the assembly (and DIFF=<kernel> prints that kernel's unified diff)
        kn = {}                                        # every kernel of NEW: name -> (unit, body, numbers)
        for unit in units:
            kn.update({k: (unit,) + v for k, v in kernels(new, unit, os.path.join(td, "new")).items()})
        used = set()
        for unit in units:
            ko = kernels(old, unit, os.path.join(td, "old"))
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
                    print(f"   MISSING  {name}"); bad = 1; continue
                used.add(match)
                (body, res), (unit_n, body_n, res_n) = ko[name], kn[match]
                same = body == body_n
                if not same and os.environ.get("DIFF") == name:
                    print("\n".join(difflib.unified_diff(body, body_n, lineterm="", n=2)))
                bad |= not same
                note = (f"  (now {match})" if match != name else "") + (f"  (now in {unit_n})" if unit_n != unit else "")
                if not same:
                    note += (f"  [{len(body_n)} lines now; opcode multiset {'equal' if ops(body) == ops(body_n) else 'DIFFERENT'}; "
                             f"VGPR / SGPR / scratch / LDS {' / '.join(map(str, res))} -> {' / '.join(map(str, res_n))}]")
                print(f"   {'identical' if same else 'DIFFERS  '} {len(body):6d} lines  {name}{note}")
        for name in sorted(set(kn) - used):
            print(f"   new      {len(kn[name][1]):6d} lines  {name}  ({kn[name][0]})")
    sys.exit(bad)


if __name__ == "__main__":
    main()
