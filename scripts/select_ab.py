"""A/B timing of the entries that run the radix select, one build of libolsr.so against another in ONE process.

    python scripts/select_ab.py --parent <libolsr.so of the parent commit> [--new <libolsr.so>] [--rounds N] [--out PATH]

The parent's library is loaded twice (parent_a; parent_b from a copy of the file, so that the loader maps it again) and the
new one once.  Legs, each timed between its own pair of device events, the three libraries alternating inside every round
and the order rotating from round to round:
  median_depth         olsr_median_depth on the 1200 x 680 depth and opacity of scripts/bench_frontend.py
  grad_mask_blocks     olsr_grad_mask, block mode, on that script's image
  grad_mask_global     the same, global mode
  keyframe_seed_plan   olsr_keyframe_seed_plan on the frame of scripts/bench_keyframe_seed.py, factor 32
Criterion per leg: the parent's spread is the interval of the medians of its groups of `group` consecutive rounds, both
copies together; the new build's median over all rounds is reported against it.  These entries take a fraction of a
millisecond on a shared host, so the parent against itself is the only honest margin.  Every output of the new build is
compared with the parent's, bit for bit.  Prints one JSON line and writes profiles/select_ab.json."""
import argparse
import ctypes as C
import json
import math
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from online_lang_splatting_amd import _abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--new", default=os.path.join(ROOT, "online_lang_splatting_amd", "libolsr.so"))
ap.add_argument("--rounds", type=int, default=60)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--group", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_ab.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("select_ab.py needs the GPU: nothing here can be measured without one")
dev = torch.device("cuda:0")
vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t


def load(path):
    L = C.CDLL(path)
    L.olsr_frontend_scratch_bytes.argtypes, L.olsr_frontend_scratch_bytes.restype = [i64], sz
    L.olsr_grad_mask.argtypes, L.olsr_grad_mask.restype = [i32, i32, i64, i32, C.c_float, vp, vp, vp, vp], C.c_int
    L.olsr_median_depth.argtypes, L.olsr_median_depth.restype = [i64] + [vp] * 7, C.c_int
    L.olsr_keyframe_seed_scratch_bytes.argtypes, L.olsr_keyframe_seed_scratch_bytes.restype = [i32, i32], sz
    L.olsr_keyframe_seed_plan.argtypes = [C.POINTER(_abi.OlsrKeyframeSeedParams), vp, vp, vp, vp,
                                          C.POINTER(_abi.OlsrMapBuffers), vp, vp, vp, vp, vp]
    L.olsr_keyframe_seed_plan.restype = C.c_int
    return L


tmp = tempfile.mkdtemp()
copy = shutil.copy(args.parent, os.path.join(tmp, "libolsr_parent_b.so"))
libs = {"parent_a": load(os.path.abspath(args.parent)), "parent_b": load(copy), "new": load(os.path.abspath(args.new))}

W, H = 1200, 680
N = W * H
f32, i32t, u8 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.uint8)
# the front end's frame (scripts/bench_frontend.py)
g = torch.Generator().manual_seed(7)
fe_image = (torch.randint(0, 256, (3, H, W), generator=g).float() / 255.0).to(dev)
fe_depth = (torch.rand(1, H, W, generator=g) * 5.7 + 0.3).to(dev)
fe_opacity = (0.9 + 0.1 * torch.rand(1, H, W, generator=g)).to(dev)
EDGE = 4.0
# the seeding's frame (scripts/bench_keyframe_seed.py)
g = torch.Generator().manual_seed(5)
kf_image = (torch.randint(13, 244, (3, H, W), generator=g).float() / 256.0).to(dev)
kf_depth = torch.rand(H, W, generator=g) * 5.7 + 0.3
kf_depth[torch.rand(H, W, generator=g) < 0.1] = 0.0
kf_depth = kf_depth.to(dev)
ca, sa = math.cos(0.4), math.sin(0.4)
w2c = torch.tensor([[ca, 0.0, sa, 0.3], [0.0, 1.0, 0.0, -0.1], [-sa, 0.0, ca, 0.7], [0.0, 0.0, 0.0, 1.0]]).to(dev)
FACTOR, M = 32, 1
cap = N // FACTOR
seed_p = _abi.OlsrKeyframeSeedParams(W=W, H=H, plane_stride=N, M=M, downsample=FACTOR, seed=1, fx=600.0, fy=600.0, cx=599.5,
                                     cy=339.5, rgb_boundary_threshold=0.01, depth_trunc=100.0, point_size=0.05,
                                     adaptive_pointsize=1, capacity=cap)


class Side:
    """one library with buffers of its own"""

    def __init__(self, L):
        self.L = L
        self.fe_scratch = torch.empty(int(L.olsr_frontend_scratch_bytes(N)), **u8)
        self.mask = {m: torch.empty(1, H, W, **f32) for m in ("blocks", "global")}
        self.median, self.count = torch.empty(1, **f32), torch.empty(1, **i32t)
        self.kf_scratch = torch.empty(int(L.olsr_keyframe_seed_scratch_bytes(W, H)), **u8)
        self.rows = dict(means3D=torch.zeros(cap, 3, **f32), shs=torch.zeros(cap, M, 3, **f32), opacities=torch.zeros(cap, 1, **f32),
                         scales=torch.zeros(cap, 3, **f32), rotations=torch.zeros(cap, 4, **f32))
        self.pix_index, self.status, self.aux = torch.zeros(cap, **i32t), torch.zeros(8, **i32t), torch.zeros(4, **f32)
        self.buffers = _abi.OlsrMapBuffers(**{k: v.data_ptr() for k, v in self.rows.items()})

    def leg(self, name):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if name == "median_depth":
            rc = self.L.olsr_median_depth(N, fe_depth.data_ptr(), fe_opacity.data_ptr(), None, self.fe_scratch.data_ptr(),
                                          self.median.data_ptr(), self.count.data_ptr(), st)
        elif name == "keyframe_seed_plan":
            rc = self.L.olsr_keyframe_seed_plan(C.byref(seed_p), kf_image.data_ptr(), kf_depth.data_ptr(), None, w2c.data_ptr(),
                                                C.byref(self.buffers), self.pix_index.data_ptr(), self.kf_scratch.data_ptr(),
                                                self.status.data_ptr(), self.aux.data_ptr(), st)
        else:
            mode = name[len("grad_mask_"):]
            rc = self.L.olsr_grad_mask(W, H, N, _abi.GRAD_MASK_BLOCKS if mode == "blocks" else _abi.GRAD_MASK_GLOBAL, EDGE,
                                       fe_image.data_ptr(), self.mask[mode].data_ptr(), self.fe_scratch.data_ptr(), st)
        assert rc == 0, (name, rc)

    def outputs(self):
        out = {"mask_blocks": self.mask["blocks"], "mask_global": self.mask["global"], "median": self.median, "count": self.count,
               "pix_index": self.pix_index, "status": self.status, "aux": self.aux}
        out.update({k: v for k, v in self.rows.items() if k != "scales"})   # (the plan leaves the scales to finish)
        return out


LEGS = ("median_depth", "grad_mask_blocks", "grad_mask_global", "keyframe_seed_plan")
sides = {k: Side(L) for k, L in libs.items()}
names = list(sides)
ms = {leg: {k: [] for k in names} for leg in LEGS}
with torch.cuda.device(dev):
    for rnd in range(args.warmup + args.rounds):
        order = names[rnd % 3:] + names[:rnd % 3]
        for leg in LEGS:
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sides[k].leg(leg)
                e1.record()
                e1.synchronize()
                if rnd >= args.warmup:
                    ms[leg][k].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()

ref, new = sides["parent_a"].outputs(), sides["new"].outputs()
out = {"what": "the entries that run the radix select, between device events; the parent build loaded twice (parent_a, parent_b) "
               "and the new build, alternating inside each round, the order rotating",
       "device": torch.cuda.get_device_name(0), "image": [W, H], "seed_factor": FACTOR, "rounds": args.rounds,
       "warmup": args.warmup, "group": args.group,
       "new_equals_parent_bits": {k: bool(torch.equal(ref[k].view(torch.int32), new[k].view(torch.int32))) for k in ref},
       "kept_rows": int(sides["new"].status[1].item()),
       "criterion": "per leg: the parent's spread is the interval of the medians of its groups of `group` consecutive rounds, "
                    "both copies together; the new build's median of all its rounds is held against it"}


def summary(v):
    groups = [round(statistics.median(v[i:i + args.group]), 5) for i in range(0, len(v) - args.group + 1, args.group)]
    return {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5),
            "group_medians_ms": groups}


for leg in LEGS:
    row = {k: summary(ms[leg][k]) for k in names}
    both = row["parent_a"]["group_medians_ms"] + row["parent_b"]["group_medians_ms"]
    lo, hi = min(both), max(both)
    row["parent_spread_ms"] = [lo, hi]
    row["new_within_parent_spread"] = lo <= row["new"]["ms_median"] <= hi
    row["new_at_most_parent_spread_upper_end"] = row["new"]["ms_median"] <= hi
    out[leg] = row
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(out, indent=1) + "\n")
shutil.rmtree(tmp, ignore_errors=True)
