"""Two-column table of every kernel's resources in two builds made with `build --force --keep-temps`.

    python scripts/isa_table.py <csrc/_obj of build A> <csrc/_obj of build B> [-o table.json] [--label-a parent --label-b new]

Per kernel: VGPRs, SGPRs, LDS bytes, scratch bytes, occupancy (resource_usage.log) and the number of s_barrier in its ISA
(the .s files -save-temps leaves beside every object).  Prints the kernels whose figures differ; the JSON holds all of them.
"""
import argparse
import glob
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
        cur = None
        for line in open(path):
            m = re.match(r"(\w+):\s+; @", line)
            if m:
                cur = k.get((unit, m.group(1)))
                if cur is not None:
                    cur["barriers"] = 0
            elif line.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and re.match(r"\s+s_barrier\b", line):
                cur["barriers"] += 1
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("-o")
    ap.add_argument("--label-a", default="a")
    ap.add_argument("--label-b", default="b")
    g = ap.parse_args()
    a, b = read_build(g.a), read_build(g.b)
    names = demangle(sorted({m for _, m in list(a) + list(b)}))
    table = {}
    for key in sorted(set(a) | set(b)):
        row = {g.label_a: a.get(key), g.label_b: b.get(key)}
        row["equal"] = row[g.label_a] == row[g.label_b]
        name = f"{key[0]}: {names[key[1]]}"
        table[f"{key[0]}: {key[1]}" if name in table else name] = row  # (overloads: the mangled name tells them apart)
    for name, row in table.items():
        if not row["equal"]:
            print(f"{name}\n    {g.label_a}: {row[g.label_a]}\n    {g.label_b}: {row[g.label_b]}")
    print(f"{sum(r['equal'] for r in table.values())} of {len(table)} kernels have equal figures")
    if g.o:
        with open(g.o, "w") as f:
            json.dump({"fields": "vgpr, sgpr, lds bytes/block, scratch bytes/lane, occupancy waves/SIMD, s_barrier count",
                       "kernels": table}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
