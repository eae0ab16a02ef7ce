"""Static figures of the forward composite's instantiations in two builds made with `build --force --keep-temps`.

    python scripts/fwd_pair_isa.py <csrc/_obj of the parent build> <csrc/_obj of this build> [-o profiles/fwd_pair_isa.json]

Per `render_fwd_kernel` instantiation: VGPRs, SGPRs, LDS, scratch and occupancy (resource_usage.log, through isa_table.py) and
the instruction mix of its pair loop, counted in the .s file -save-temps leaves beside the object: the innermost (depth 2) loop
that holds the accumulation's v_pk_fma_f32, every block the compiler marks as part of it, from its header to its latch.
Classes: vector (v_*), LDS (ds_*), branch (s_branch, s_cbranch_*), wait (s_waitcnt), nop (s_nop), scalar (every other s_*).
The MFMA instantiations keep their accumulation outside v_pk_fma_f32; their loop is found by its v_mfma instead.
Exits 1 if an instantiation's occupancy or scratch differs between the builds, or if the default's pair loop
(<15, 15, 0, 0, false>) issues more vector instructions than the parent's or more than 62 scalar + branch instructions.
"""
import argparse
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_table  # noqa: E402

CLASSES = ("vector", "scalar", "branch", "wait", "nop", "lds")
DEFAULT = "render_fwd_kernel<15, 15, 0, 0, false>"
SCALAR_BRANCH_BOUND = 62


def classify(op):
    if op.startswith("v_"):
        return "vector"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64"):
        return "branch"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_nop":
        return "nop"
    if op.startswith("s_"):
        return "scalar"
    return None  # (global_*, buffer_*: none in the pair loop)


def pair_loops(obj):
    """mangled kernel name -> instruction mix of its pair loop"""
    out = {}
    for path in glob.glob(os.path.join(obj, "k_render_fwd*", "*-hip-amdgcn-amd-amdhsa-gfx*.s")):
        unit = os.path.basename(os.path.dirname(path))
        kernel = None
        loops = {}   # header label of a depth-2 loop -> {class: count, "_marks": accumulation instructions}
        cur = None   # the loop the current block belongs to
        for line in open(path):
            m = re.match(r"(_ZN4olsr17render_fwd_kernel\w+):\s+; @", line)
            if m:
                kernel, loops, cur = m.group(1), {}, None
                continue
            if kernel is None:
                continue
            if line.startswith(".Lfunc_end"):
                best = max((l for l in loops.values() if l["_marks"]), key=lambda l: l["vector"], default=None)
                if best is not None:
                    out[(unit, kernel)] = {c: best[c] for c in CLASSES}
                kernel = None
                continue
            lab = re.match(r"\.LBB(\d+_\d+):", line)
            if lab:
                cur = None  # (a block outside every loop carries no loop comment)
                pending = lab.group(1)
            m = re.search(r"Inner Loop Header: Depth=2", line)
            if m:
                cur = loops.setdefault(pending, dict({c: 0 for c in CLASSES}, _marks=0))
                continue
            m = re.search(r"in Loop: Header=BB(\d+_\d+) Depth=2", line)
            if m:
                cur = loops.setdefault(m.group(1), dict({c: 0 for c in CLASSES}, _marks=0))
                continue
            if re.match(r"; %bb\.", line):
                cur = None  # (a fall-through block: its own loop comment follows on this or the next line)
                m = re.search(r"Header=BB(\d+_\d+) Depth=2", line)
                if m:
                    cur = loops.setdefault(m.group(1), dict({c: 0 for c in CLASSES}, _marks=0))
                continue
            ins = re.match(r"\s+([a-z_0-9]+)\b", line)
            if ins and cur is not None:
                c = classify(ins.group(1))
                if c:
                    cur[c] += 1
                if ins.group(1).startswith(("v_pk_fma_f32", "v_mfma")):
                    cur["_marks"] += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-o")
    g = ap.parse_args()
    res = {"parent": isa_table.read_build(g.parent), "new": isa_table.read_build(g.new)}
    loops = {"parent": pair_loops(g.parent), "new": pair_loops(g.new)}
    keys = sorted(k for k in set(res["parent"]) | set(res["new"]) if "render_fwd_kernel" in k[1])
    names = isa_table.demangle(sorted({m for _, m in keys}))
    table, bad = {}, []
    for key in keys:
        row = {}
        for label in ("parent", "new"):
            r = res[label].get(key)
            row[label] = None if r is None else {**{f: r.get(f) for f in ("vgpr", "sgpr", "lds", "scratch", "occupancy")},
                                                 "pair_loop": loops[label].get(key)}
        name = f"{key[0]}: {names[key[1]]}"
        table[name] = row
        p, n = row["parent"], row["new"]
        if p is None or n is None or p["occupancy"] != n["occupancy"] or p["scratch"] != n["scratch"]:
            bad.append(f"{name}: occupancy / scratch {p and (p['occupancy'], p['scratch'])} -> {n and (n['occupancy'], n['scratch'])}")
        if names[key[1]] == DEFAULT and p and n and p["pair_loop"] and n["pair_loop"]:
            lp, ln = p["pair_loop"], n["pair_loop"]
            print(f"{name}\n  parent {lp}\n  new    {ln}")
            if ln["vector"] > lp["vector"]:
                bad.append(f"{name}: {ln['vector']} vector instructions per pair, parent {lp['vector']}")
            if ln["scalar"] + ln["branch"] > SCALAR_BRANCH_BOUND:
                bad.append(f"{name}: {ln['scalar']} + {ln['branch']} scalar + branch instructions per pair, bound {SCALAR_BRANCH_BOUND}")
    for name, row in table.items():
        p, n = row["parent"], row["new"]
        if p and n:
            lp, ln = p["pair_loop"] or {}, n["pair_loop"] or {}
            print(f"{name}: vgpr {p['vgpr']}->{n['vgpr']} sgpr {p['sgpr']}->{n['sgpr']} lds {p['lds']}->{n['lds']} scratch "
                  f"{p['scratch']}->{n['scratch']} occ {p['occupancy']}->{n['occupancy']} | v {lp.get('vector')}->{ln.get('vector')} "
                  f"s {lp.get('scalar')}->{ln.get('scalar')} br {lp.get('branch')}->{ln.get('branch')} "
                  f"lds {lp.get('lds')}->{ln.get('lds')} wait {lp.get('wait')}->{ln.get('wait')}")
    if g.o:
        with open(g.o, "w") as f:
            json.dump({"fields": "per build: vgpr, sgpr, lds bytes/block, scratch bytes/lane, occupancy waves/SIMD; pair_loop: "
                                 "instructions of the pair loop from header to latch by class (vector v_*, scalar s_* without "
                                 "branches, s_waitcnt and s_nop, branch, wait, nop, lds ds_*)",
                       "bound": {"kernel": DEFAULT, "scalar_plus_branch_at_most": SCALAR_BRANCH_BOUND,
                                 "vector": "no more than the parent's"},
                       "kernels": table, "violations": bad}, f, indent=1)
            f.write("\n")
    for b in bad:
        print("VIOLATION", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
