"""gaussian_map.MapSpec — the torch specification of the map edits — against the reference's own GaussianModel
(tests/golden/map_edit.npz <- tests/golden/make_golden_map_edit.py), bit for bit on the CPU, stage by stage: parameters,
both Adam moments, per-group step counts, kfIDs, n_obs and the accumulators."""
import json
import os

import numpy as np
import pytest
import torch

import map_edit_case as case
from online_lang_splatting_amd.gaussian_map import GROUPS, MapSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_edit.npz")


class SpecOps:
    """The case's operations on a MapSpec (what make_golden_map_edit.Ops does on a GaussianModel)."""

    def __init__(self):
        self.src = {}

    def step(self, m, grads, skip):
        m.step(grads, skip)

    def stats(self, m, views):
        dev = m.max_radii.device
        for grad, vis, radii in views:
            m.update_max_radii(radii.to(dev), vis.to(dev))
            m.add_densification_stats(grad.to(dev), vis.to(dev))

    def densify(self, m, args, z):
        self.src["densify"] = m.densify_and_prune(*args, z=z.to(m.max_radii.device))

    def reset_nonvisible(self, m, filters):
        m.reset_opacity_nonvisible([f.to(m.max_radii.device) for f in filters])

    def prune(self, m, mask):
        self.src["prune"] = m.prune(mask.to(m.max_radii.device))

    def extend(self, m, rows, kf_id):
        dev = m.max_radii.device
        self.src["extend"] = m.extend(*(rows[k].to(dev) for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")),
                                      kf_id)


def initial_spec(device="cpu"):
    init = case.initial_map(torch.Generator().manual_seed(case.SEED - 1))
    return MapSpec(*(init[n].to(device) for n in GROUPS), lrs=case.LRS, kf_id=init["kf_id"].to(device),
                   n_obs=init["n_obs"].to(device), percent_dense=case.PERCENT_DENSE)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return json.loads(str(z["digests"])), z


@pytest.fixture(scope="module")
def played():
    spec = initial_spec()
    ops = SpecOps()
    got = {}
    states = {}

    def record(stage, m):
        st = m.export()
        got[stage] = case.digests(st)
        states[stage] = {k: v.clone() for k, v in st.items()}
    case.run(spec, ops, record)
    return got, states, ops


@pytest.mark.parametrize("stage", case.STAGES)
def test_spec_reproduces_reference_stage(golden, played, stage):
    want, _ = golden
    got, states, _ = played
    bad = [k for k in want[stage] if want[stage][k] != got[stage].get(k)]
    assert not bad, f"stage {stage}: {bad} differ from the reference's GaussianModel (P = {states[stage]['means3D'].shape[0]})"


def test_densify_full_arrays(golden, played):
    """The recorded arrays after densify_and_prune, element by element (a readable failure where a digest only says 'no')."""
    _, z = golden
    _, states, _ = played
    st = states["densify"]
    for k, v in st.items():
        ref = torch.from_numpy(z[f"densify_{k}"])
        assert tuple(ref.shape) == tuple(v.shape), (k, ref.shape, v.shape)
        assert torch.equal(v.cpu(), ref), k


def test_every_branch_is_exercised(played):
    """The case is only a test if clones, splits, world-space prunes, opacity prunes and 0/0 statistics all occur."""
    _, states, ops = played
    src = ops.src["densify"]
    P0 = case.P0
    counts = np.bincount(src.numpy(), minlength=P0)
    assert (counts == 0).any()          # dropped or split-and-removed
    assert (counts == 2).any()          # kept original + clone, or two children
    before = states["stats1"]
    st = before["stats"]
    assert bool((st[:, 1] == 0).any()) and bool((st[:, 1] > 0).any())
    # per-group steps: the opacity group lags after the reset
    steps = states["densify_init"]["group_steps"].tolist()
    assert steps[GROUPS.index("opacity")] == steps[0] - 1
    # extend: appended rows carry the negative codes
    ext = ops.src["extend"]
    assert int((ext < 0).sum()) == case.N_NEW and int(ext[-1]) == -case.N_NEW
