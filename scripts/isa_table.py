"""Table of every kernel's resources in two (or, with --mid, three) builds made with `build --force --keep-temps`.

    python scripts/isa_table.py <csrc/_obj of build A> <csrc/_obj of build B> [-o table.json] [--label-a parent --label-b new]
                                 [--rename-a REGEX REPL] [--mid <csrc/_obj of a build between A and B> --label-mid step]

Per kernel: VGPRs, SGPRs, LDS bytes, scratch bytes, occupancy (resource_usage.log) and the number of s_barrier in its ISA
(the .s files -save-temps leaves beside every object), and the SHA-256 of its instruction stream: the kernel's lines of the .s
file without comments and blank lines, without the __hip_cuid_* symbol (a hash of the source text) and with the function index
taken out of local labels (.LBB<n>_: it shifts when a kernel earlier in the file goes) and the kernel's own symbol replaced by
a placeholder (its descriptor, which names it, is part of the stream; a renamed kernel still compares).  Equal hashes: the same
machine code.
--rename-a maps the (demangled) kernel names of build A onto build B's where a kernel was renamed.  A kernel that moved to
another unit under its own name is paired by that name.  --mid adds a column for an
intermediate build (named like B); a row is equal when all of its columns are.
Prints the kernels whose figures differ; the JSON holds all of them.
"""
import argparse
import glob
import hashlib
import json
import os
import re
import subprocess

FIELDS = {"VGPRs": "vgpr", "TotalSGPRs": "sgpr", "LDS Size [bytes/block]": "lds", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy"}


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    out = p.stdout.split("\n") if p.returncode == 0 else names
    # (the name without its parameter list; "(anonymous namespace)::" is no parameter list)
    short = {m: re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "").split("(")[0].replace("olsr::", "")
             for m, d in zip(names, out)}
    return {m: s or m for m, s in short.items()}


def read_build(obj):
    k = {}
    unit = cur = None
    for line in open(os.path.join(obj, "resource_usage.log")):
        if line.startswith("==== "):
            unit = line.split()[1][:-2]
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = k.setdefault((unit, m.group(1)), {})
            continue
        m = re.search(r":\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    for path in glob.glob(os.path.join(obj, "*", "*-hip-amdgcn-amd-amdhsa-gfx*.s")):
        unit = os.path.basename(os.path.dirname(path))
        cur = stream = own = None
        for line in open(path):
            m = re.match(r"(\w+):\s+; @", line)
            if m:
                cur = k.get((unit, m.group(1)))
                if cur is not None:
                    cur["barriers"] = 0
                    stream, own = hashlib.sha256(), m.group(1)
            elif line.startswith(".Lfunc_end"):  # (the .amdhsa_kernel descriptor sits in front of it: part of the stream)
                if cur is not None:
                    cur["stream_sha256"] = stream.hexdigest()
                cur = None
            elif cur is not None:
                if re.match(r"\s+s_barrier\b", line):
                    cur["barriers"] += 1
                text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).replace(own, "<kernel>").strip()
                if text and "__hip_cuid_" not in text:
                    stream.update(text.encode() + b"\n")
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("-o")
    ap.add_argument("--label-a", default="a")
    ap.add_argument("--label-b", default="b")
    ap.add_argument("--rename-a", nargs=2, metavar=("REGEX", "REPL"))
    ap.add_argument("--mid")
    ap.add_argument("--label-mid", default="mid")
    g = ap.parse_args()
    a, b, mid = read_build(g.a), read_build(g.b), read_build(g.mid) if g.mid else {}
    names = demangle(sorted({m for _, m in list(a) + list(b) + list(mid)}))

    def by_name(build, rename):
        out = {}
        for key in sorted(build):
            short = re.sub(rename[0], rename[1], names[key[1]]) if rename else names[key[1]]
            name = f"{key[0]}: {short}"
            out[f"{key[0]}: {key[1]}" if name in out else name] = build[key]  # (overloads: the mangled name tells them apart)
        return out

    col_a, col_b = by_name(a, g.rename_a), by_name(b, None)
    # a kernel of A whose unit is gone from B pairs with the one kernel of that name in B that has no partner of its own
    for name in [n for n in col_a if n not in col_b]:
        moved = [n for n in col_b if n not in col_a and n.split(": ", 1)[1] == name.split(": ", 1)[1]]
        if len(moved) == 1:
            col_a[moved[0]] = col_a.pop(name)
    cols = [(g.label_a, col_a)]
    cols += [(g.label_mid, by_name(mid, None))] if g.mid else []
    cols += [(g.label_b, col_b)]
    table = {}
    for name in sorted(set().union(*(c for _, c in cols))):
        row = {label: c.get(name) for label, c in cols}
        row["equal"] = all(v == row[g.label_a] for v in row.values())
        table[name] = row
    for name, row in table.items():
        if not row["equal"]:
            print(name + "".join(f"\n    {label}: {row[label]}" for label, _ in cols))
    print(f"{sum(r['equal'] for r in table.values())} of {len(table)} kernels have equal figures")
    if g.o:
        with open(g.o, "w") as f:
            json.dump({"fields": "vgpr, sgpr, lds bytes/block, scratch bytes/lane, occupancy waves/SIMD, s_barrier count, "
                                 "SHA-256 of the normalised instruction stream",
                       "kernels": table}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
