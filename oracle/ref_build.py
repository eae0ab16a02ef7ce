"""Builds the reference rasterisers' own kernel sources as host C++ (oracle/_ref/libref_t{tile}_f{F}.so for the plain
rasteriser DGR, oracle/_ref/libref_dgrd_t16_f{F}.so for the disentangled one DGR-D).  TEST INFRASTRUCTURE ONLY.

The reference's cuda_rasterizer/{forward,backward,rasterizer_impl}.cu compile unmodified with g++ once the CUDA headers
they include are answered by oracle/ref_shim/ (an execution model: fibers that meet at every barrier, blocks in ascending
order, the project's pinned exp).  This recipe

  1. copies cuda_rasterizer/*.cu and *.h from the reference tree into oracle/_ref/src/t{tile}_f{F}/;
  2. applies two text rules, both regular expressions over token shapes:
       `name<targs> <<< cfg >>> (`  ->  `REF_LAUNCH((name<targs>), cfg)(`      (a macro of the shim)
       `#define BLOCK_X|BLOCK_Y|NUM_LANGUAGE_CHANNELS <n>` in the copied config.h  ->  the build's values;
  3. compiles the three sources, the shim's scheduler and oracle/ref_entry.cpp (a C ABI of our own over the reference's
     Rasterizer / LanguageRasterizer entry points) with the oracle's flags.

The second family, DGR-D (submodules/diff-gaussian-rasterization-disentangle-optim, its own cuda_rasterizer/ and
third_party/glm), goes through the same two rules and the same shim unmodified; only the entry file differs
(oracle/ref_entry_dgrd.cpp: DGR-D's LanguageRasterizer takes both parameter sets and two binning buffers).  Its sources
are copied to oracle/_ref/src/dgrd_t16_f{F}/.

Nothing under oracle/_ref/ is committed: the copies and the libraries are build products that hold the reference's text.
The reference tree is found the way tests/golden/make_golden_*.py find it (/root/reference; OLSR_REFERENCE_ROOT overrides).

usage: python oracle/ref_build.py [--san]     (--san: the stand-alone sanitised program of `make -C oracle ref_san`)
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
REF_ROOT = os.environ.get("OLSR_REFERENCE_ROOT", "/root/reference")
REF_DGR = os.path.join(REF_ROOT, "submodules", "diff-gaussian-rasterization")
REF_SRC = os.path.join(REF_DGR, "cuda_rasterizer")
REF_GLM = os.path.join(REF_DGR, "third_party", "glm")

REF_DGRD = os.path.join(REF_ROOT, "submodules", "diff-gaussian-rasterization-disentangle-optim")

# (tile, F): the shipped configuration first.  F = 0 runs through the RGB entry points of any of them.
BUILDS = ((15, 15), (16, 15), (15, 3), (15, 16))
# DGR-D: its tile with its shipped channel count, and with the product's
DGRD_BUILDS = ((16, 3), (16, 15))
UNITS = ("forward.cu", "backward.cu", "rasterizer_impl.cu")
# the oracle's own flags (oracle/Makefile), minus OpenMP: nothing runs in parallel inside a launch
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math"]
SAN = ["-fsanitize=undefined,address,float-cast-overflow", "-fno-sanitize-recover=all"]

# kernel name with optional template arguments, then `<<<` (written `<< <` in places), the launch configuration,
# `>>>` (`>> >`), and the opening parenthesis of the argument list
LAUNCH = re.compile(r"([A-Za-z_]\w*(?:\s*<[^<>;(){}]*>)?)\s*<\s*<\s*<(.*?)>\s*>\s*>\s*\(", re.S)
MIN_LAUNCH_SITES = 10  # (the three sources hold 15 today; fewer than ten means the rule no longer sees them)


class Family:
    """One reference source tree: where it lies, how its copies and libraries are named, its entry file."""

    def __init__(self, name, root, prefix, entry, min_sites, builds):
        self.name, self.prefix, self.entry, self.min_sites, self.builds = name, prefix, entry, min_sites, builds
        self.src = os.path.join(root, "cuda_rasterizer")
        self.glm = os.path.join(root, "third_party", "glm")

    def present(self):
        return os.path.isdir(self.src) and os.path.isdir(self.glm)


DGR = Family("dgr", REF_DGR, "", "ref_entry.cpp", MIN_LAUNCH_SITES, BUILDS)
# (DGR-D's three sources hold 18 launch sites today)
DGRD = Family("dgrd", REF_DGRD, "dgrd_", "ref_entry_dgrd.cpp", 13, DGRD_BUILDS)


def have_reference(fam=DGR):
    return fam.present()


def lib_path(tile, F, libm_exp=False, fam=DGR):
    return os.path.join(OUT, f"libref_{fam.prefix}t{tile}_f{F}{'_libmexp' if libm_exp else ''}.so")


def existing_builds(fam=DGR):
    return [(t, f) for (t, f) in fam.builds if os.path.exists(lib_path(t, f, fam=fam))]


def _rewrite_launches(text):
    return LAUNCH.subn(lambda m: f"REF_LAUNCH(({' '.join(m.group(1).split())}), {m.group(2).strip()})(", text)


def _set_define(text, name, value):
    text, n = re.subn(rf"^([ \t]*#[ \t]*define[ \t]+{name}[ \t]+)\d+", rf"\g<1>{value}", text, flags=re.M)
    assert n == 1, f"config.h: expected one #define {name} <number>, found {n}"
    return text


def copy_sources(tile, F, fam=DGR):
    """oracle/_ref/src/[dgrd_]t{tile}_f{F}/: the family's sources with the two text rules applied.  Returns the directory."""
    dst = os.path.join(OUT, "src", f"{fam.prefix}t{tile}_f{F}")
    os.makedirs(dst, exist_ok=True)
    sites = 0
    for name in sorted(os.listdir(fam.src)):
        if not name.endswith((".cu", ".h")):
            continue
        text = open(os.path.join(fam.src, name), encoding="utf-8", errors="surrogateescape").read()
        if name.endswith(".cu"):
            text, n = _rewrite_launches(text)
            sites += n
            assert "<<<" not in re.sub(r"\s", "", text), f"{name}: a launch site survived the rewrite"
        if name == "config.h":
            for key, val in (("BLOCK_X", tile), ("BLOCK_Y", tile), ("NUM_LANGUAGE_CHANNELS", F)):
                text = _set_define(text, key, val)
        out = os.path.join(dst, name)
        if not (os.path.exists(out) and open(out, encoding="utf-8", errors="surrogateescape").read() == text):
            with open(out, "w", encoding="utf-8", errors="surrogateescape") as f:
                f.write(text)
    assert sites >= fam.min_sites, f"{fam.name}: only {sites} launch sites rewritten"
    return dst


def _compile_cmd(src_dir, extra, out, sources, shared, fam=DGR):
    # -iquote, not -I, for the copied sources: they hold a file named math.h that must answer `#include "math.h"` only
    cmd = [os.environ.get("CXX", "g++")] + FLAGS + extra
    # Several builds are loaded into one process.  The block-wide statics of the kernel templates have vague linkage, which
    # g++ marks STB_GNU_UNIQUE: the loader would then give the 16 x 16 build the 15 x 15 build's 225-entry arrays.
    # -fno-gnu-unique and -Bsymbolic keep every library on its own definitions.
    cmd += ["-shared", "-fno-gnu-unique", "-Wl,-Bsymbolic"] if shared else []
    cmd += ["-iquote", src_dir, "-I", os.path.join(HERE, "ref_shim"), "-I", fam.glm, "-I", os.path.join(HERE, "..", "include")]
    for s in sources:
        cmd += (["-x", "c++", s] if s.endswith(".cu") else ["-x", "none", s])
    return cmd + ["-o", out]


def _sources(src_dir, fam=DGR):
    return [os.path.join(src_dir, u) for u in UNITS] + [os.path.join(HERE, "ref_shim", "ref_exec.cpp"),
                                                        os.path.join(HERE, fam.entry)]


def _stale(out, deps):
    return (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _deps(src_dir, fam=DGR):
    shim = os.path.join(HERE, "ref_shim")
    d = [os.path.join(r, f) for r, _, fs in os.walk(shim) for f in fs]
    d += [os.path.join(src_dir, f) for f in os.listdir(src_dir)]
    return d + [os.path.join(HERE, fam.entry), os.path.join(HERE, "pinned_exp.h"), os.path.abspath(__file__)]


def build_one(tile, F, libm_exp=False, verbose=False, fam=DGR):
    src_dir = copy_sources(tile, F, fam)
    out = lib_path(tile, F, libm_exp, fam)
    if _stale(out, _deps(src_dir, fam)):
        cmd = _compile_cmd(src_dir, ["-DREF_LIBM_EXP"] if libm_exp else [], out, _sources(src_dir, fam), shared=True,
                           fam=fam)
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


def build_all(verbose=False):
    """The four builds of the plain rasteriser and the two of DGR-D, compiled side by side.  Returns their paths."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OUT, exist_ok=True)
    jobs = [(DGR, b) for b in BUILDS] + [(DGRD, b) for b in DGRD_BUILDS if DGRD.present()]
    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        return list(ex.map(lambda j: build_one(*j[1], verbose=verbose, fam=j[0]), jobs))


def build_san(verbose=True):
    """oracle/_ref/ref_san_main (tile 15, F 15): copied sources + shim + ref_san_main.cpp under UBSan and ASan."""
    os.makedirs(OUT, exist_ok=True)
    src_dir = copy_sources(15, 15)
    out = os.path.join(OUT, "ref_san_main")
    cmd = _compile_cmd(src_dir, ["-O1", "-g"] + SAN, out, _sources(src_dir) + [os.path.join(HERE, "ref_san_main.cpp")],
                       shared=False)
    cmd = [c for c in cmd if c not in ("-O2", "-fPIC")]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    if not have_reference():
        sys.exit(f"reference tree not found under {REF_ROOT}")
    if "--san" in sys.argv[1:]:
        print(build_san())
    else:
        for p in build_all(verbose="-v" in sys.argv[1:]):
            print(p)
