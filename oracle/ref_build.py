"""Builds the reference rasteriser's own kernel sources as host C++ (oracle/_ref/libref_t{tile}_f{F}.so).
TEST INFRASTRUCTURE ONLY.

The reference's cuda_rasterizer/{forward,backward,rasterizer_impl}.cu compile unmodified with g++ once the CUDA headers
they include are answered by oracle/ref_shim/ (an execution model: fibers that meet at every barrier, blocks in ascending
order, the project's pinned exp).  This recipe

  1. copies cuda_rasterizer/*.cu and *.h from the reference tree into oracle/_ref/src/t{tile}_f{F}/;
  2. applies two text rules, both regular expressions over token shapes:
       `name<targs> <<< cfg >>> (`  ->  `REF_LAUNCH((name<targs>), cfg)(`      (a macro of the shim)
       `#define BLOCK_X|BLOCK_Y|NUM_LANGUAGE_CHANNELS <n>` in the copied config.h  ->  the build's values;
  3. compiles the three sources, the shim's scheduler and oracle/ref_entry.cpp (a C ABI of our own over the reference's
     Rasterizer / LanguageRasterizer entry points) with the oracle's flags.

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

# (tile, F): the shipped configuration first.  F = 0 runs through the RGB entry points of any of them.
BUILDS = ((15, 15), (16, 15), (15, 3), (15, 16))
UNITS = ("forward.cu", "backward.cu", "rasterizer_impl.cu")
# the oracle's own flags (oracle/Makefile), minus OpenMP: nothing runs in parallel inside a launch
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math"]
SAN = ["-fsanitize=undefined,address,float-cast-overflow", "-fno-sanitize-recover=all"]

# kernel name with optional template arguments, then `<<<` (written `<< <` in places), the launch configuration,
# `>>>` (`>> >`), and the opening parenthesis of the argument list
LAUNCH = re.compile(r"([A-Za-z_]\w*(?:\s*<[^<>;(){}]*>)?)\s*<\s*<\s*<(.*?)>\s*>\s*>\s*\(", re.S)
MIN_LAUNCH_SITES = 10  # (the three sources hold 15 today; fewer than ten means the rule no longer sees them)


def have_reference():
    return os.path.isdir(REF_SRC) and os.path.isdir(REF_GLM)


def lib_path(tile, F, libm_exp=False):
    return os.path.join(OUT, f"libref_t{tile}_f{F}{'_libmexp' if libm_exp else ''}.so")


def existing_builds():
    return [(t, f) for (t, f) in BUILDS if os.path.exists(lib_path(t, f))]


def _rewrite_launches(text):
    return LAUNCH.subn(lambda m: f"REF_LAUNCH(({' '.join(m.group(1).split())}), {m.group(2).strip()})(", text)


def _set_define(text, name, value):
    text, n = re.subn(rf"^([ \t]*#[ \t]*define[ \t]+{name}[ \t]+)\d+", rf"\g<1>{value}", text, flags=re.M)
    assert n == 1, f"config.h: expected one #define {name} <number>, found {n}"
    return text


def copy_sources(tile, F):
    """oracle/_ref/src/t{tile}_f{F}/: the reference's sources with the two text rules applied.  Returns the directory."""
    dst = os.path.join(OUT, "src", f"t{tile}_f{F}")
    os.makedirs(dst, exist_ok=True)
    sites = 0
    for name in sorted(os.listdir(REF_SRC)):
        if not name.endswith((".cu", ".h")):
            continue
        text = open(os.path.join(REF_SRC, name), encoding="utf-8", errors="surrogateescape").read()
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
    assert sites >= MIN_LAUNCH_SITES, f"only {sites} launch sites rewritten"
    return dst


def _compile_cmd(src_dir, extra, out, sources, shared):
    # -iquote, not -I, for the copied sources: they hold a file named math.h that must answer `#include "math.h"` only
    cmd = [os.environ.get("CXX", "g++")] + FLAGS + extra
    # Several builds are loaded into one process.  The block-wide statics of the kernel templates have vague linkage, which
    # g++ marks STB_GNU_UNIQUE: the loader would then give the 16 x 16 build the 15 x 15 build's 225-entry arrays.
    # -fno-gnu-unique and -Bsymbolic keep every library on its own definitions.
    cmd += ["-shared", "-fno-gnu-unique", "-Wl,-Bsymbolic"] if shared else []
    cmd += ["-iquote", src_dir, "-I", os.path.join(HERE, "ref_shim"), "-I", REF_GLM, "-I", os.path.join(HERE, "..", "include")]
    for s in sources:
        cmd += (["-x", "c++", s] if s.endswith(".cu") else ["-x", "none", s])
    return cmd + ["-o", out]


def _sources(src_dir):
    return [os.path.join(src_dir, u) for u in UNITS] + [os.path.join(HERE, "ref_shim", "ref_exec.cpp"),
                                                        os.path.join(HERE, "ref_entry.cpp")]


def _stale(out, deps):
    return (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _deps(src_dir):
    shim = os.path.join(HERE, "ref_shim")
    d = [os.path.join(r, f) for r, _, fs in os.walk(shim) for f in fs]
    d += [os.path.join(src_dir, f) for f in os.listdir(src_dir)]
    return d + [os.path.join(HERE, "ref_entry.cpp"), os.path.join(HERE, "pinned_exp.h"), os.path.abspath(__file__)]


def build_one(tile, F, libm_exp=False, verbose=False):
    src_dir = copy_sources(tile, F)
    out = lib_path(tile, F, libm_exp)
    if _stale(out, _deps(src_dir)):
        cmd = _compile_cmd(src_dir, ["-DREF_LIBM_EXP"] if libm_exp else [], out, _sources(src_dir), shared=True)
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


def build_all(verbose=False):
    """The four reference builds, compiled side by side.  Returns their paths."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OUT, exist_ok=True)
    with ThreadPoolExecutor(max_workers=len(BUILDS)) as ex:
        return list(ex.map(lambda b: build_one(*b, verbose=verbose), BUILDS))


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
