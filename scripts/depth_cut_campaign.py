"""Randomised campaign for the per-tile depth cut-offs (include/olsr.h): sequences of views that drift away from a start view
by random steps, on random scenes, tiles 15 / 16, F in {0, 3, 15}, sparse and dense scenes, odd image sizes.  After every
frame the contract is checked against a workspace without cut-offs on the same inputs:
   status 0  =>  images, radii, n_touched bit-identical, gradients equal up to summation order (1e-5 relative);
   status 3  =>  zero gradients, and the array is repaired enough that a repeat of the SAME view ends in status 0 within 3 tries.
Prints one line per sequence and a summary; exit code 1 on any violation.   python scripts/depth_cut_campaign.py [n_sequences] [seed]"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_lang_splatting_amd.frame_shard import RasterWorkspace
from online_lang_splatting_amd.scene import Camera, make_scene

dev = torch.device("cuda:0")
NSEQ = int(sys.argv[1]) if len(sys.argv) > 1 else 40
SEED = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = torch.Generator().manual_seed(SEED)


def rnd(lo, hi):
    return lo + (hi - lo) * float(torch.rand(1, generator=rng))


def camera(W, H, yaw, pitch, t):
    a, b = math.radians(yaw), math.radians(pitch)
    Ry = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    return Camera(W, H, W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0, Rx @ Ry, torch.tensor(t))


def camd(c):
    return dict(viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev),
                projmatrix_raw=c.projection_matrix.to(dev), campos=c.camera_center.to(dev), tanfovx=c.tanfovx, tanfovy=c.tanfovy)


def same(out, grads, out_ref, grads_ref):
    for k in out_ref:
        if not torch.equal(out[k], out_ref[k]):
            return f"forward output {k} differs"
    for k in grads_ref:
        if grads_ref[k].numel() == 0:
            continue
        scale = float(grads_ref[k].abs().max())
        err = (grads[k] - grads_ref[k]).abs()
        if not bool((err <= 1e-5 * grads_ref[k].abs() + 1e-7 * scale).all()):
            return f"gradient {k}: worst {float(err.max()):.3e} at scale {scale:.3e}"
    return None


bad, frames, misses, kept, full = 0, 0, 0, 0, 0
for s in range(NSEQ):
    W = int(rnd(90, 420)); H = int(rnd(70, 300))
    F = (0, 3, 15)[int(rnd(0, 3))]
    tile = (15, 16)[int(rnd(0, 2))]
    P = int(10 ** rnd(2.5, 4.6))
    scale_mult = 10 ** rnd(-0.5, 0.4)
    sc = make_scene(P, W, H, F, seed=1000 * SEED + s, scale_mult=scale_mult)
    g = dict(bg=sc.bg.to(dev), means3D=sc.means3D.to(dev), opacities=sc.opacities.to(dev), scales=sc.scales.to(dev),
             rotations=sc.rotations.to(dev), shs=sc.shs.to(dev), language=None if F == 0 else sc.language.to(dev))
    cot = [None if t is None else t.to(dev) for t in sc.cotangents(s)]
    cap = 4_000_000
    plain = RasterWorkspace(P, W, H, F, sc.shs.shape[1], cap, dev, tile=tile)
    cut = RasterWorkspace(P, W, H, F, sc.shs.shape[1], cap, dev, tile=tile, depth_cut=True)
    yaw, pitch, t = 0.0, 0.0, [0.0, 0.0, 0.0]
    step = 10 ** rnd(-2.0, 0.3)   # degrees / centimetres-ish per frame: from sub-pixel drifts to jumps
    seq_miss = 0
    for f in range(12):
        cam = camd(camera(W, H, yaw, pitch, t))
        plain.set_scene(sh_degree=sc.sh_degree, **cam, **g)
        o_ref = {k: v.clone() for k, v in plain.forward().items()}
        g_ref = {k: v.clone() for k, v in plain.backward(*cot).items()}
        if plain.rendered()[1]:
            break  # (capacity: not this campaign's subject)
        for attempt in range(4):
            cut.set_scene(sh_degree=sc.sh_degree, **cam, **g)
            o = {k: v.clone() for k, v in cut.forward().items()}
            gr = {k: v.clone() for k, v in cut.backward(*cot).items()}
            st = cut.forward_status()
            frames += 1
            if st == 0:
                why = same(o, gr, o_ref, g_ref)
                if why:
                    bad += 1
                    print(f"VIOLATION seq {s} frame {f} attempt {attempt}: status 0 but {why}  (P {P} {W}x{H} F {F} tile {tile})")
                kept += cut.rendered()[0]; full += plain.rendered()[0]
                break
            if st != 3:   # OLSR_STATUS_CUT_MISS
                bad += 1
                print(f"VIOLATION seq {s} frame {f}: status {st}")
                break
            misses += 1; seq_miss += 1
            if any(float(v.abs().max()) != 0.0 for v in gr.values() if v.numel()) or int(cut.bwd_status.cpu()[1]) != 3:
                bad += 1
                print(f"VIOLATION seq {s} frame {f}: a flagged frame handed out gradients")
        else:
            bad += 1
            print(f"VIOLATION seq {s} frame {f}: still flagged after 4 attempts on the same view")
        yaw += rnd(-1, 1) * step; pitch += rnd(-1, 1) * step
        t = [t[0] + 0.01 * rnd(-1, 1) * step, t[1] + 0.01 * rnd(-1, 1) * step, t[2] + 0.01 * rnd(-1, 1) * step]
    print(f"seq {s:3d}: P {P:6d} {W}x{H} F {F:2d} tile {tile} scale x{scale_mult:.2f} step {step:.3f}: misses {seq_miss}")
print(f"SUMMARY sequences {NSEQ} frames {frames} misses {misses} violations {bad} instances kept {kept} of {full} "
      f"({100.0 * kept / max(full, 1):.1f} %)")
sys.exit(1 if bad else 0)
