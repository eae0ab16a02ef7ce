"""MappingStep on a GaussianMap: the back end's loop with map edits between and inside its iterations, on a small room scene —
iterations -> densify_and_prune (in the iteration's hook, before the step) -> iterations -> reset_opacity_nonvisible -> the
co-visibility prune of a full window -> extend (a new keyframe's rows) -> iterations.

The same sequence runs on the torch specification (gaussian_map.MapSpec, whose optimiser is torch.optim.Adam) fed the SAME
GPU gradients and statistics the fused path produced.  Identical: P, src_index of every edit, kfID, n_obs, the statistics and
the per-group step counts (the skipped step of the densify iteration, the opacity group's lag after the reset).

Parameters and moments are NOT held bit for bit, which departs from the issue that asked for it: they are held to the
tolerance tests/test_gpu_api.py holds FusedAdam to torch.optim.Adam (rtol 1e-5, atol 1e-6).  torch's GPU Adam kernels
contract multiply-adds and round their own way, and the difference compounds over the loop's ten steps.  Measured on an
MI355X (the test prints it): max distance 26 ulp in means3D, 2 in scales, 59 in opacities, 4 in exp_avg_sq; up to 3.3e3
ulp in rotations / language and 7e4 in exp_avg, on elements that cancel to near zero (about 20 % of exp_avg differs in
the last bits at all).  The edits themselves move rows exactly (tests/test_gpu_map_edit.py, bit for bit against the same
specification).  With carry_order=True the run is bit-identical to the run with fresh sorts: the carried depth order is
dropped at every resize and the lists never depend on it."""
import pytest
import torch

from online_lang_splatting_amd.frame_shard import FrameLanes
from online_lang_splatting_amd.gaussian_map import GROUPS, GaussianMap, MapSpec
from online_lang_splatting_amd.scene import make_room_scene
from online_lang_splatting_amd.slam_iterations import MappingStep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)
SPEC_LRS = dict(xyz=LRS["xyz"], f_dc=LRS["sh_dc"], f_rest=LRS["sh_rest"], opacity=LRS["opacity"], scaling=LRS["scale"],
                rotation=LRS["rotation"], f_language=LRS["language"])
DENSIFY_AT, RESET_AT, PRUNE_AT, EXTEND_AFTER, ITERS = 3, 6, 8, 8, 12


def run(carry_order, with_spec):
    W, H, F, views = 320, 184, 15, 6
    rs = make_room_scene(24_000, W, H, F, views=views, seed=5)
    sc = rs.scene
    dev = torch.device(DEV)
    P = sc.P
    kf = torch.repeat_interleave(torch.arange(len(rs.points_per_keyframe), dtype=torch.int32), torch.tensor(rs.points_per_keyframe))[:P]
    raw = dict(means3D=sc.means3D, shs=sc.shs, opacities=torch.logit(sc.opacities), scales=torch.log(sc.scales),
               rotations=sc.rotations, language=sc.language)
    m = GaussianMap(*(raw[k].to(dev).contiguous() for k in ("means3D", "shs", "opacities", "scales", "rotations", "language")),
                    LRS, kf_id=kf.to(dev), device=dev)
    spec = None
    if with_spec:
        spec = MapSpec(raw["means3D"].to(dev), raw["shs"][:, :1].to(dev), raw["shs"][:, 1:].to(dev), raw["opacities"].to(dev),
                       raw["scales"].to(dev), raw["rotations"].to(dev), raw["language"].to(dev), SPEC_LRS, kf_id=kf.to(dev))
    camd = [dict(viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev),
                 projmatrix_raw=c.projection_matrix.to(dev), campos=c.camera_center.to(dev), tanfovx=c.tanfovx,
                 tanfovy=c.tanfovy) for c in rs.cameras]
    lanes = FrameLanes(1, P, W, H, F, 1, 600_000, dev)
    g = torch.Generator().manual_seed(17)
    log = dict(src=[], P=[])
    it = {"i": 0}
    # about half the map on either side of the clone / split size (off the median itself, which would sit on the threshold)
    extent = float(torch.exp(raw["scales"]).max(dim=1).values.median()) / 0.01 * 1.00037

    def hook(step, total):
        i = it["i"]
        grads = None
        if spec is not None:
            flat = total.flat
            sl = m.layout.slices()
            grads = dict(xyz=flat[:, sl["means3D"]], f_dc=flat[:, sl["sh"]][:, :3], f_rest=flat[:, sl["sh"]][:, 3:],
                         opacity=flat[:, sl["opacity"]], scaling=flat[:, sl["scales"]], rotation=flat[:, sl["rotations"]],
                         f_language=flat[:, sl["language"]])
            grads = {k: v.clone() for k, v in grads.items()}
            if i != PRUNE_AT:
                spec.add_bucket_stats(total.densify, total.max_radii)
        skip = ()
        if i == DENSIFY_AT:
            z = torch.randn(m.P, 2, 3, generator=g).to(dev)
            log["src"].append(m.densify_and_prune(2e-4, 0.2, extent, 20, z=z))
            if spec is not None:
                log.setdefault("spec_src", []).append(spec.densify_and_prune(2e-4, 0.2, extent, 20, z=z))
            skip = "all"
        elif i == RESET_AT:
            filters = list(step.visibility.values())
            m.reset_opacity_nonvisible(filters)
            if spec is not None:
                spec.reset_opacity_nonvisible(filters)
            skip = ("opacity",)
        elif i == PRUNE_AT:
            vis = [step.touched[v] for v in range(views)]
            log["src"].append(m.covisibility_prune(vis, list(range(views)), mode="slam"))
            if spec is not None:
                log.setdefault("spec_src", []).append(spec.covisibility_prune(vis, list(range(views)), mode="slam"))
            skip = "all"
        if spec is not None:
            spec.step(grads, skip)
        return None

    ms = MappingStep(lanes, None, sc.bg.to(dev), 0, camd, rs.targets, LRS, exposure=torch.zeros(2, device=dev),
                     fused_loss=True, carry_order=carry_order, gaussian_map=m, edit_hook=hook, record_visibility=True)
    for i in range(ITERS):
        it["i"] = i
        ms.iteration(stats=(i != PRUNE_AT))
        log["P"].append(m.P)
        if i == EXTEND_AFTER:   # a new keyframe's Gaussians between two mapping calls
            n = 700
            idx = torch.randint(0, m.P, (n,), generator=g).to(dev)
            jit = (torch.randn(n, 3, generator=g) * 0.01).to(dev)
            rows = dict(means3D=m.params["means3D"][idx] + jit, shs=m.params["shs"][idx].clone(),
                        opacities=torch.zeros(n, 1, device=dev), scales=m.params["scales"][idx].clone(),
                        rotations=m.params["rotations"][idx].clone())
            log["src"].append(m.extend(**rows, kf_id=len(rs.points_per_keyframe)))
            if spec is not None:
                log.setdefault("spec_src", []).append(
                    spec.extend(rows["means3D"], rows["shs"][:, :1], rows["shs"][:, 1:], rows["opacities"], rows["scales"],
                                rows["rotations"], len(rs.points_per_keyframe)))
        assert not any(ws.rendered()[1] for ws, _, _ in lanes.lanes)
    torch.cuda.synchronize()
    return m, spec, log


def ulps(a, b):
    """Distance in units in the last place between two fp32 tensors (the integers of their ordered bit patterns)."""
    def key(t):
        i = t.view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def test_mapping_with_edits_equals_specification(hip):
    m, spec, log = run(carry_order=False, with_spec=True)
    P = log["P"]
    assert P[DENSIFY_AT] != P[0] and P[PRUNE_AT] < P[PRUNE_AT - 1] and P[EXTEND_AFTER + 1] == P[EXTEND_AFTER] + 700, P
    for a, b in zip(log["src"], log["spec_src"]):
        assert torch.equal(a.cpu().long(), b.cpu().long())
    got, want = m.state(), spec.export()
    assert got["group_steps"].tolist() == want["group_steps"].tolist()
    steps = got["group_steps"].tolist()
    assert steps[GROUPS.index("opacity")] == steps[0] - 1 and steps[0] == ITERS - 2, steps
    for k in ("kf_id", "n_obs"):
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    assert torch.equal(got["stats"].cpu(), want["stats"].cpu())
    assert torch.equal(got["max_radii"].cpu(), want["max_radii"].cpu().int())
    spread = {}
    for k in ("means3D", "shs", "opacities", "scales", "rotations", "language", "exp_avg", "exp_avg_sq"):
        a, b = got[k].detach().cpu().contiguous(), want[k].detach().cpu().reshape(got[k].shape).contiguous()
        spread[k] = (int(ulps(a, b).max()) if a.numel() else 0, int((a != b).sum()), a.numel())
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=lambda s, k=k: f"{k}: {s}")
    print("parameters / moments against torch.optim.Adam (max ulp, elements differing, elements):", spread)


def test_carried_order_follows_the_edits(hip):
    a, _, la = run(carry_order=False, with_spec=False)
    b, _, lb = run(carry_order=True, with_spec=False)
    assert la["P"] == lb["P"]
    for x, y in zip(la["src"], lb["src"]):
        assert torch.equal(x, y)
    sa, sb = a.state(), b.state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
