"""Time of one map edit on the device (GaussianMap.densify_and_prune / prune_points: olsr_map_edit_plan + the one host read +
olsr_map_edit_apply) against the torch specification (gaussian_map.MapSpec: the reference's own torch expressions and optimiser
surgery) on the same GPU, at the config-3 shape (500 k Gaussians, F = 15, M = 1) and on the room map (scene.make_room_scene).

    python scripts/bench_map_edit.py [--P 500000] [--reps 20] [--room] [--no-torch] [--json OUT]

The synthetic map is built so that about 5 % of the rows clone, 5 % split and 10 % are dropped.  Reported per edit: the
median device-event time of the whole call (host read included), the rows of each segment, the bytes the apply moves (every
source row read once, every destination row written once) and that traffic over the HBM copy rate of MI355X_MICROARCH.md
(~6.3 TB/s) — the floor.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python
scripts/bench_map_edit.py --reps 5` run.

Measured on one MI355X (500 k Gaussians, F = 15, M = 1; 5 % clone, 5 % split, 10 % dropped; medians of 20 edits):
  densify_and_prune  0.275 ms per edit (room map 0.264 ms); torch specification 6.92 ms (6.89 ms)
  prune_points       0.206 ms per edit (room map 0.207 ms); torch specification 1.69 ms (1.63 ms)
  kernels (rocprofv3): map_edit_apply 162 us on average (135 - 189 us), map_edit_classify 6.8 us, map_edit_prefix 6.9 us
  traffic: 369 MB per densify edit, 59 us at the HBM copy rate
The 0.15 ms budget is not met: the apply kernel runs at about a third of the copy rate (one thread per element of the
[11 + 3M + F] row, a branch per parameter array and up to four destination rows per element: narrow, partly scattered
stores), and the host read of P_new between the two launches adds its round trip to the event time."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from online_lang_splatting_amd.gaussian_map import GaussianMap, MapSpec  # noqa: E402

LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)
SPEC_LRS = dict(xyz=LRS["xyz"], f_dc=LRS["sh_dc"], f_rest=LRS["sh_rest"], opacity=LRS["opacity"], scaling=LRS["scale"],
                rotation=LRS["rotation"], f_language=LRS["language"])
HBM_BPS = 6.3e12


def synthetic_state(P, M, F, seed=0, base=None):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(P, generator=g)
    # 5 % clone (high gradient, small), 5 % split (high gradient, large), 10 % low opacity, the rest kept
    smax = torch.where(u < 0.05, torch.full((P,), 0.005), torch.where(u < 0.10, torch.full((P,), 0.03), torch.full((P,), 0.006)))
    grad = torch.where(u < 0.10, torch.full((P,), 1e-3), torch.full((P,), 1e-5))
    op = torch.where((u >= 0.10) & (u < 0.20), torch.full((P,), -3.0), torch.full((P,), 3.0))
    W = 11 + 3 * M + F
    st = dict(means3D=torch.randn(P, 3, generator=g), shs=torch.randn(P, M, 3, generator=g), opacities=op.view(P, 1),
              scales=torch.log(smax).view(P, 1).repeat(1, 3), rotations=torch.randn(P, 4, generator=g),
              language=torch.randn(P, F, generator=g), exp_avg=torch.randn(P, W, generator=g) * 1e-3,
              exp_avg_sq=torch.rand(P, W, generator=g) * 1e-6, kf_id=torch.randint(0, 9, (P,), generator=g).int(),
              n_obs=torch.zeros(P, dtype=torch.int32), stats=torch.stack([grad * 2, torch.full((P,), 2.0)], 1),
              max_radii=torch.zeros(P, dtype=torch.int32), group_steps=torch.full((7,), 10, dtype=torch.int64))
    if base is not None:   # real geometry (the room map), synthetic statistics
        for k in ("means3D", "shs", "rotations", "language"):
            st[k] = base[k].reshape(st[k].shape)
    return st, torch.randn(P, 2, 3, generator=g)


def spec_of(st, dev):
    return MapSpec.from_state(st, SPEC_LRS, dev)


def time_call(fn, reps, setup):
    ms = []
    for _ in range(reps):
        obj = setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(obj)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def moved_bytes(P, status, M, F, mode):
    W = 11 + 3 * M + F
    per_row_read = (W + 2 * W) * 4 + (8 if mode == "densify" else 8 + 8 + 4) + 1
    if mode == "densify":
        per_row_read += 8   # stats read by the plan
    P_new = status[0]
    per_row_write = (W + 2 * W) * 4 + 8 + 8 + 4 + 4
    return P * per_row_read + P_new * per_row_write


def leg(name, st, z, dev, reps, with_torch, M, F):
    P = st["means3D"].shape[0]
    out = {"leg": name, "P": P}
    for mode in ("densify", "prune"):
        mask = (torch.rand(P, generator=torch.Generator().manual_seed(1)) < 0.1).to(dev)

        def setup():
            return GaussianMap.from_state(st, LRS, dev)

        def run(m):
            if mode == "densify":
                m.densify_and_prune(2e-4, 0.5, 1.0, 20, z=zd)
            else:
                m.prune_points(mask)
        zd = z.to(dev)
        med, all_ms = time_call(run, reps, setup)
        m = setup()
        run(m)
        status = m.status.cpu().tolist()
        nbytes = moved_bytes(P, status, M, F, mode)
        r = dict(ms_median=round(med, 4), ms_all=[round(x, 4) for x in all_ms], P_new=status[0], kept=status[1],
                 clones=status[2], split_children=2 * status[3], bytes_moved=nbytes,
                 hbm_floor_ms=round(nbytes / HBM_BPS * 1e3, 4))
        if with_torch:
            def tsetup():
                return spec_of(st, dev)

            def trun(s):
                if mode == "densify":
                    s.densify_and_prune(2e-4, 0.5, 1.0, 20, z=zd)
                else:
                    s.prune(mask)
            tmed, _ = time_call(trun, max(3, reps // 4), tsetup)
            r["torch_spec_ms_median"] = round(tmed, 4)
        out[mode] = r
        del m
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=500_000)
    ap.add_argument("--M", type=int, default=1)
    ap.add_argument("--F", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--room", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(gpu=torch.cuda.get_device_name(0), legs=[])
    st, z = synthetic_state(a.P, a.M, a.F)
    res["legs"].append(leg("synthetic", st, z, dev, a.reps, not a.no_torch, a.M, a.F))
    print(json.dumps(res["legs"][-1]), flush=True)
    if a.room:
        from online_lang_splatting_amd.scene import make_room_scene
        rs = make_room_scene(a.P, 1200, 680, a.F, views=10, seed=3)
        sc = rs.scene
        base = dict(means3D=sc.means3D, shs=sc.shs, rotations=sc.rotations, language=sc.language)
        st, z = synthetic_state(sc.P, 1, a.F, base=base)
        res["legs"].append(leg("room", st, z, dev, a.reps, not a.no_torch, 1, a.F))
        print(json.dumps(res["legs"][-1]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
