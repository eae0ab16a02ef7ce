"""The map-edit primitive of the library (olsr_map_edit_plan / _apply, csrc/k_map_edit.hip) behind GaussianMap, against the
torch specification (gaussian_map.MapSpec) and, through it, the reference's GaussianModel (tests/golden/map_edit.npz).

Identical: masks (which rows survive), order, src_index, every copied row, both moments, kfID, n_obs, accumulators, step
counts.  Split children: xyz and scaling within 2^-20 of the row's largest coordinate — they are computed from exp / log /
a 3x3 product (a coordinate of xyz + R (std z) can cancel to near zero and keep the terms' absolute rounding), and
torch's exp / log / bmm on the CPU (the fixture) or the GPU (its own kernels, which round differently and may contract) are
not the operation sequence a kernel can be held to bit for bit; every other field of a child is a raw copy and identical."""
import numpy as np
import pytest
import torch

import map_edit_case as case
from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.gaussian_map import GROUPS, GaussianMap, MapSpec
from test_map_edit_cpu import SpecOps, initial_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED_LRS = dict(xyz=case.LRS["xyz"], sh_dc=case.LRS["f_dc"], sh_rest=case.LRS["f_rest"], opacity=case.LRS["opacity"],
                 scale=case.LRS["scaling"], rotation=case.LRS["rotation"], language=case.LRS["f_language"])
CHILD_RTOL = 2.0 ** -20


def children_rows(m):
    """Destination rows that are split children: [kept + clones, P_new - appended)."""
    st = m.status.cpu().tolist()
    return st[1] + st[2], st[0] - st[4]


def compare(m, want, src_index=None, want_src=None, what=""):
    got = m.state()
    c0, c1 = children_rows(m)
    assert got["means3D"].shape[0] == want["means3D"].shape[0], (what, got["means3D"].shape, want["means3D"].shape)
    if want_src is not None:
        assert torch.equal(src_index.cpu().long(), want_src.cpu().long()), f"{what}: src_index"
    for k in ("means3D", "shs", "opacities", "scales", "rotations", "language", "exp_avg", "exp_avg_sq", "kf_id", "n_obs",
              "stats", "group_steps"):
        a, b = got[k].detach().cpu(), want[k].detach().cpu().to(got[k].dtype).reshape(got[k].shape)
        if k in ("means3D", "scales") and c1 > c0:
            # (relative to the row's largest coordinate: a child's xyz is xyz + R (std z), and a coordinate where the two
            #  terms cancel to near zero keeps the absolute error of the terms, not a relative one)
            ca, cb = a[c0:c1], b[c0:c1]
            tol = CHILD_RTOL * cb.abs().amax(dim=1, keepdim=True)
            err = (ca - cb).abs()
            assert bool((err <= tol).all()), f"{what} {k} children: {int((err > tol).sum())} beyond 2^-20 of the row, worst " \
                                             f"{float((err / tol.clamp_min(1e-30)).max()) * CHILD_RTOL:.3g}"
            a = torch.cat([a[:c0], a[c1:]])
            b = torch.cat([b[:c0], b[c1:]])
        assert torch.equal(a, b), f"{what}: {k} differs ({int((a != b).sum())} elements)"
    assert torch.equal(got["max_radii"].cpu(), want["max_radii"].cpu().to(torch.int32)), f"{what}: max_radii"


@pytest.fixture(scope="module")
def stages():
    """The CPU specification's state before and after every stage of the fixture's case (it reproduces the reference bit
    for bit: tests/test_map_edit_cpu.py), with the edits' inputs."""
    spec, out, inputs = initial_spec(), {}, {}

    def snap(m):   # (export() shares the parameters' storage, which later steps update in place)
        return {k: v.clone() for k, v in m.export().items()}

    class Recording(SpecOps):
        def densify(self, m, args, z):
            inputs.setdefault("densify", []).append((snap(m), args, z))
            super().densify(m, args, z)

        def reset_nonvisible(self, m, filters):
            inputs["reset"] = (snap(m), filters)
            super().reset_nonvisible(m, filters)
            inputs["reset_after"] = snap(m)

        def prune(self, m, mask):
            inputs["prune"] = (snap(m), mask)
            super().prune(m, mask)

        def extend(self, m, rows, kf_id):
            inputs["extend"] = (snap(m), rows, kf_id)
            super().extend(m, rows, kf_id)
    ops = Recording()

    def record(stage, m):
        out[stage] = snap(m)
        out[stage + ":src"] = m.src.clone()
    case.run(spec, ops, record)
    return out, inputs


def test_densify_stages_match_reference(hip, stages):
    out, inputs = stages
    for (before, args, z), stage in zip(inputs["densify"], ("densify", "densify_init")):
        m = GaussianMap.from_state(before, FUSED_LRS, DEV, percent_dense=case.PERCENT_DENSE)
        src = m.densify_and_prune(*args, z=z.to(DEV))
        compare(m, out[stage], src, out[stage + ":src"], stage)
        # the reference's next optimizer.step() updates nothing
        assert m.pending_skip == set(GROUPS)


def test_reset_prune_extend_match_reference(hip, stages):
    out, inputs = stages
    before, filters = inputs["reset"]
    m = GaussianMap.from_state(before, FUSED_LRS, DEV)
    m.reset_opacity_nonvisible([f.to(DEV) for f in filters])
    compare(m, inputs["reset_after"], what="reset_opacity_nonvisible")
    assert m.pending_skip == {"opacity"}
    before, mask = inputs["prune"]
    m = GaussianMap.from_state(before, FUSED_LRS, DEV)
    src = m.prune_points(mask.to(DEV))
    compare(m, out["prune"], src, out["prune:src"], "prune_points")
    before, rows, kf = inputs["extend"]
    m = GaussianMap.from_state(before, FUSED_LRS, DEV)
    shs = torch.cat([rows["f_dc"], rows["f_rest"]], dim=1)
    src = m.extend(rows["xyz"], shs, rows["opacity"], rows["scaling"], rows["rotation"], kf)
    compare(m, out["extend"], src, out["extend:src"], "extend")


def test_growing_past_the_back_buffer(hip):
    """The second set of buffers exists and is too small for the edit: it is replaced, the result is the specification's."""
    st, _ = random_map(3001, 1, 15, seed=21)
    m = GaussianMap.from_state(st, FUSED_LRS, DEV, capacity=3001)
    spec = spec_from_state(st, DEV)
    mask = torch.rand(3001, generator=torch.Generator().manual_seed(2)) < 0.1
    src, want = m.prune_points(mask.to(DEV)), spec.prune(mask.to(DEV))                           # allocates the back set
    compare(m, spec.export(), src, want, "prune")
    small = m._bufs[1 - m._front]
    assert small is not None and small["cap"] == 3001
    rows = random_map(700, 1, 15, seed=22)[0]                                                     # 2700 + 700 > 3001
    src = m.extend(rows["means3D"], rows["shs"], rows["opacities"], rows["scales"], rows["rotations"], kf_id=4)
    want = spec.extend(rows["means3D"].to(DEV), rows["shs"][:, :1].to(DEV), rows["shs"][:, 1:].to(DEV),
                       rows["opacities"].to(DEV), rows["scales"].to(DEV), rows["rotations"].to(DEV), 4)
    assert m.capacity > 3001 and m.P == spec.P > 3001
    compare(m, spec.export(), src, want, "extend past the back buffer")


# ---- random maps ------------------------------------------------------------------------------------------------------
def random_map(P, M, F, seed, margin=True):
    g = torch.Generator().manual_seed(seed)
    smax = torch.exp(torch.empty(P).uniform_(np.log(0.002), np.log(0.3), generator=g))
    if margin:   # no decision within 1e-3 relative of a threshold (0.01 clone / split, 0.1 world size, 0.16 for children)
        for thr in (0.01, 0.1, 0.16):
            near = (smax - thr).abs() < 2e-3 * thr
            smax[near] = thr * 1.01
    ratio = torch.cat([torch.ones(P, 1), 0.3 + 0.7 * torch.rand(P, 2, generator=g)], 1)
    op = torch.where(torch.rand(P, generator=g) < 0.1, torch.empty(P).uniform_(-3, 0.5, generator=g),
                     torch.empty(P).uniform_(1.2, 4, generator=g))
    accum = torch.exp(torch.empty(P).uniform_(np.log(1e-5), np.log(1e-3), generator=g))
    denom = torch.randint(0, 4, (P,), generator=g).float()
    accum = torch.where(denom > 0, accum * denom, torch.zeros(P))
    gr = accum / denom
    near = (gr - 2e-4).abs() < 2e-3 * 2e-4
    accum[near] *= 1.1
    f_dc = torch.randn(P, 1, 3, generator=g)
    f_rest = torch.randn(P, max(M - 1, 0), 3, generator=g) * 0.1
    st = dict(means3D=torch.randn(P, 3, generator=g) * 3, shs=torch.cat([f_dc, f_rest], 1) if M else torch.zeros(P, 0, 3),
              opacities=op.view(P, 1), scales=torch.log(smax.view(P, 1) * ratio), rotations=torch.randn(P, 4, generator=g),
              language=torch.randn(P, F, generator=g), exp_avg=torch.randn(P, 11 + 3 * M + F, generator=g) * 1e-3,
              exp_avg_sq=torch.rand(P, 11 + 3 * M + F, generator=g) * 1e-6, kf_id=torch.randint(0, 9, (P,), generator=g).int(),
              n_obs=torch.randint(0, 6, (P,), generator=g).int(), stats=torch.stack([accum, denom], 1),
              max_radii=torch.randint(0, 40, (P,), generator=g).int(), group_steps=torch.full((7,), 11, dtype=torch.int64))
    return st, torch.randn(P, 2, 3, generator=g)


def spec_from_state(st, device):
    return MapSpec.from_state(st, case.LRS, device)


@pytest.mark.parametrize("P,M,F", [(200_003, 1, 15), (500_001, 1, 15), (70_001, 16, 0), (65_537, 1, 16)])
def test_random_maps_densify_and_prune(hip, P, M, F):
    st, z = random_map(P, M, F, seed=P + M + F)
    spec = spec_from_state(st, DEV)
    want_src = spec.densify_and_prune(2e-4, 0.7, 1.0, 20, z=z.to(DEV))
    m = GaussianMap.from_state(st, FUSED_LRS, DEV)
    src = m.densify_and_prune(2e-4, 0.7, 1.0, 20, z=z.to(DEV))
    counts = m.status.cpu().tolist()
    assert counts[2] > 0 and counts[3] > 0 and counts[1] + counts[3] < P, counts   # clones, splits and drops
    compare(m, spec.export(), src, want_src, f"P={P} M={M} F={F}")
    # a prune by mask on the result, with the accumulators following the rows (the specification restarts from the map's own
    # state: the split children's xyz / scaling above agree to 2^-20, not to the bit)
    spec = spec_from_state({k: v.detach().cpu() for k, v in m.state().items()}, DEV)
    mask = torch.rand(m.P, generator=torch.Generator().manual_seed(5)) < 0.1
    want_src = spec.prune(mask.to(DEV))
    src = m.prune_points(mask.to(DEV))
    compare(m, spec.export(), src, want_src, f"prune P={P}")


def test_edge_cases(hip):
    # nothing selected: 0/0 statistics everywhere, opaque, small -> the identity
    st, z = random_map(4099, 1, 15, seed=3)
    st["stats"].zero_()
    st["opacities"].fill_(3.0)
    st["scales"].clamp_(max=-3.0)
    m = GaussianMap.from_state(st, FUSED_LRS, DEV)
    src = m.densify_and_prune(2e-4, 0.7, 1.0, 20, z=z.to(DEV))
    assert torch.equal(src.cpu(), torch.arange(4099, dtype=torch.int32))
    assert torch.equal(m.params["means3D"].cpu(), st["means3D"]) and torch.equal(m.adam.exp_avg.cpu(), st["exp_avg"])
    assert int(m.stats.abs().sum()) == 0 and int(m.max_radii.abs().sum()) == 0   # zeroed by the postfix
    # everything dropped: P_new = 0, then the empty map grows again
    st, z = random_map(1000, 1, 15, seed=4)
    m = GaussianMap.from_state(st, FUSED_LRS, DEV)
    src = m.densify_and_prune(2e-4, 1.0, 1.0, 20, z=z.to(DEV))
    assert m.P == 0 and src.numel() == 0
    r = random_map(17, 1, 15, seed=6)[0]
    src = m.extend(r["means3D"], r["shs"], r["opacities"], r["scales"], r["rotations"], kf_id=3)
    assert m.P == 17 and torch.equal(src.cpu(), -1 - torch.arange(17, dtype=torch.int32))
    assert torch.equal(m.params["means3D"].cpu(), r["means3D"]) and int(m.params["language"].abs().sum()) == 0
    assert bool((m.kf_id == 3).all()) and int(m.n_obs.abs().sum()) == 0 and int(m.adam.exp_avg.abs().sum()) == 0


def test_two_runs_are_bit_identical(hip):
    st, z = random_map(300_007, 1, 15, seed=9)
    res = []
    for _ in range(2):
        m = GaussianMap.from_state(st, FUSED_LRS, DEV)
        src = m.densify_and_prune(2e-4, 0.7, 1.0, 20, z=z.to(DEV))
        res.append((src.cpu(), {k: v.detach().cpu().clone() for k, v in m.state().items()}))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_adam_groups_entry(hip):
    """olsr_adam_step_groups: equal steps and no skip == olsr_adam_step (bit for bit); a skipped group is untouched and its
    lagging step count gives the bias corrections of torch.optim.Adam's per-parameter step."""
    from online_lang_splatting_amd.frame_shard import FusedAdam, GradLayout, GradientBucket
    P, M, F = 4097, 1, 15
    st, _ = random_map(P, M, F, seed=12)
    lay = GradLayout(M, F)
    bucket = GradientBucket(P, lay, DEV)
    bucket.flat.copy_(torch.randn(P, lay.width, generator=torch.Generator().manual_seed(1)).to(DEV) * 1e-3)
    outs = []
    for groups in (False, True):
        m = GaussianMap.from_state(st, FUSED_LRS, DEV)
        if groups:   # force the per-group entry with equal counts
            m.adam.group_steps = [11] * 7
            gp = _abi.OlsrAdamGroupParams()
            import ctypes as C
            from online_lang_splatting_amd._lib import check, lib
            hp = _abi.OlsrAdamParams(lr_xyz=FUSED_LRS["xyz"], lr_sh_dc=FUSED_LRS["sh_dc"], lr_sh_rest=FUSED_LRS["sh_rest"],
                                     lr_opacity=FUSED_LRS["opacity"], lr_scale=FUSED_LRS["scale"],
                                     lr_rotation=FUSED_LRS["rotation"], lr_language=FUSED_LRS["language"], beta1=0.9,
                                     beta2=0.999, eps=1e-15, step=1)
            gp.base = hp
            for i in range(7):
                gp.group_step[i] = 12
            flats = (C.c_void_p * 1)(bucket.flat.data_ptr())
            p = m.params
            check(lib().olsr_adam_step_groups(P, M, F, C.byref(gp), 1, flats, None, p["means3D"].data_ptr(),
                                              p["shs"].data_ptr(), p["opacities"].data_ptr(), p["scales"].data_ptr(),
                                              p["rotations"].data_ptr(), p["language"].data_ptr(),
                                              m.adam.exp_avg.data_ptr(), m.adam.exp_avg_sq.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        else:
            m.step([bucket])
        outs.append({k: v.detach().cpu().clone() for k, v in m.state().items()})
    for k in ("means3D", "shs", "opacities", "scales", "rotations", "language", "exp_avg", "exp_avg_sq"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    # skip the opacity group: untouched; the others step as before
    m = GaussianMap.from_state(st, FUSED_LRS, DEV)
    m.reset_opacity()
    op = m.params["opacities"].clone()
    m.step([bucket])
    assert torch.equal(m.params["opacities"], op) and int(m.adam.exp_avg[:, 3 + 3 * M].abs().sum()) == 0
    assert m.group_steps == [12, 12, 12, 11, 12, 12, 12]
    assert torch.equal(m.params["means3D"].cpu(), outs[0]["means3D"])
    # the next step: opacity at its own step 12, the rest at 13 == torch.optim.Adam with per-parameter counts
    spec = spec_from_state({k: v.cpu() for k, v in m.state().items()}, "cpu")
    assert spec.group_steps() == [12, 12, 12, 11, 12, 12, 12]
    m.step([bucket])
    g = bucket.flat.cpu()
    sl = lay.slices()
    grads = dict(xyz=g[:, sl["means3D"]], f_dc=g[:, sl["sh"]][:, :3], f_rest=g[:, sl["sh"]][:, 3:],
                 opacity=g[:, sl["opacity"]], scaling=g[:, sl["scales"]], rotation=g[:, sl["rotations"]],
                 f_language=g[:, sl["language"]])
    spec.step(grads)
    want = spec.export()
    assert m.group_steps == want["group_steps"].tolist()
    for k in ("means3D", "opacities", "scales", "rotations", "language"):
        # (torch's CPU Adam fuses some multiply-adds: one ulp, as tests/test_gpu_api.py allows)
        torch.testing.assert_close(m.params[k].cpu(), want[k], rtol=2e-6, atol=2e-7)
