"""Per-kernel digest of hipcc -S --cuda-device-only output: python tools/kisa.py file.s [file.s ...] [--diff other.txt]

One line per kernel, sorted by mangled name: the name, a hash of its instruction stream and the resources tools/kres.py prints.
The instruction stream is the text from the kernel's label to its .Lfunc_end, without comments and "; %bb" lines, and with the
function index of local labels (.LBB<n>_<m>: the kernel's position in its file) taken out — so a kernel that moves between files
keeps its line as long as its machine code is the same.  --diff FILE compares the lines with a listing made earlier and exits 1
when the two sets differ.  The tool hashes and compares whole streams; it does not look at what the instructions are."""
import hashlib, re, sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"^    \.%s:\s+(\S+)" % k, blk, re.M) or [None, "?"])[1]
        name = g("name")
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), txt, re.M | re.S)
        if not m:
            raise SystemExit(f"{path}: no body for {name}")
        lines = []
        for ln in m.group(0).splitlines()[1:-1]:
            ln = ln.split(";", 1)[0].rstrip()
            if ln.strip():
                lines.append(re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", ln))
        h = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
        out[name] = (f"{name} isa {h} lines {len(lines)} vgpr {g('vgpr_count')} sgpr {g('sgpr_count')} lds {g('group_segment_fixed_size')} "
                     f"scratch {g('private_segment_fixed_size')} spill {g('vgpr_spill_count')}")
    return out


def main():
    args, ref = sys.argv[1:], None
    if "--diff" in args:
        i = args.index("--diff")
        ref = args[i + 1]
        del args[i:i + 2]
    lines = {}
    for p in args:
        for name, ln in kernels(p).items():
            if name in lines:
                raise SystemExit(f"{name} appears twice")
            lines[name] = ln
    got = [lines[k] for k in sorted(lines)]
    if ref is None:
        print("\n".join(got))
        return 0
    want = [ln.rstrip("\n") for ln in open(ref) if " isa " in ln]
    bad = sorted(set(got) ^ set(want))
    for ln in bad:
        print(("- " if ln in want else "+ ") + ln)
    print(f"{len(got)} kernels here, {len(want)} in {ref}: " + ("identical" if not bad else f"{len(bad)} lines differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
