"""adam_step_kernel (csrc/k_adam.hip) behind olsr_adam_step / _sum / _masked / _groups and frame_shard.FusedAdam, against
tests/adam_ref.py: the unfused float32 sequence of torch's single-tensor Adam.  Equality is a == b or both NaN, the sign of zero
included, on parameters, exp_avg and exp_avg_sq after EVERY step.  The build (-ffp-contract=off, correctly rounded divide and
sqrt, float32 denormals kept) makes that the expectation, not a tolerance.  tests/test_adam_ref_cpu.py ties the restatement to
torch.optim.Adam and shows that these inputs tell each of a table of wrong kernels from the right one."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as A
from online_lang_splatting_amd import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = ("means3D", "shs", "opacities", "scales", "rotations", "language")


def _split(flat, M, F):
    """[P, width] in the bucket's column layout -> the six parameter tensors on the GPU (contiguous, each its own storage)."""
    P = flat.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(flat))
    c = 3 + 3 * M
    parts = dict(means3D=t[:, :3], shs=t[:, 3:c].reshape(P, M, 3), opacities=t[:, c:c + 1], scales=t[:, c + 1:c + 4],
                 rotations=t[:, c + 4:c + 8], language=t[:, c + 8:])
    return {k: v.contiguous().to(DEV) for k, v in parts.items()}


def _join(params):
    P = params["means3D"].shape[0]
    return torch.cat([params[k].reshape(P, -1) for k in PARAMS], dim=1).cpu().numpy()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() > 0 else None   # (M = 0 / F = 0: NULL, as the entries allow)


def _hp(case, step):
    lr = case.lrs
    return _abi.OlsrAdamParams(lr_xyz=lr[0], lr_sh_dc=lr[1], lr_sh_rest=lr[2], lr_opacity=lr[3], lr_scale=lr[4], lr_rotation=lr[5],
                               lr_language=lr[6], beta1=0.9, beta2=0.999, eps=1e-15, step=step)


def _mask_tensor(words):
    return torch.from_numpy(words.view(np.int64).copy()).to(DEV)


def _call_entry(case, s, params, m, v):
    """One step through the C entry the case names."""
    from online_lang_splatting_amd._lib import check, lib
    flats_t = [torch.from_numpy(b).to(DEV) for b in s.buckets]
    masks_t = [None if (s.masks is None or w is None) else _mask_tensor(w) for w in (s.masks or [None] * len(flats_t))]
    flats = (C.c_void_p * len(flats_t))(*[t.data_ptr() for t in flats_t])
    masks = (C.c_void_p * len(flats_t))(*[t.data_ptr() if t is not None else None for t in masks_t])
    tail = [_ptr(params[k]) for k in PARAMS] + [m.data_ptr(), v.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    P, M, F = case.P, case.M, case.F
    if case.entry == "step":
        assert len(flats_t) == 1 and s.masks is None
        check(lib().olsr_adam_step(P, M, F, C.byref(_hp(case, s.step)), flats_t[0].data_ptr(), *tail))
    elif case.entry == "sum":
        assert s.masks is None
        check(lib().olsr_adam_step_sum(P, M, F, C.byref(_hp(case, s.step)), len(flats_t), flats, *tail))
    elif case.entry == "masked":
        check(lib().olsr_adam_step_masked(P, M, F, C.byref(_hp(case, s.step)), len(flats_t), flats, masks, *tail))
    else:
        gp = _abi.OlsrAdamGroupParams(base=_hp(case, 1), skip_mask=sum(1 << g for g in s.skip))
        for g in range(7):
            gp.group_step[g] = s.group_steps[g]
        check(lib().olsr_adam_step_groups(P, M, F, C.byref(gp), len(flats_t), flats, masks if s.masks is not None else None, *tail))
    torch.cuda.synchronize()   # (the buckets and masks are this call's own tensors)


def _assert_same(label, got, want):
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq"), got, want):
        same = A.same_bits(a, b)
        if not same.all():
            r, c = np.argwhere(~same)[0]
            raise AssertionError(f"{label}: {name} differ from the restatement on {int((~same).sum())} of {same.size} elements, first at "
                                 f"row {r} column {c}: kernel {a[r, c]!r} ({a[r, c].view(np.uint32):#010x}), restatement "
                                 f"{b[r, c]!r} ({np.float32(b[r, c]).view(np.uint32):#010x})")


def _run_entries(case):
    """The case through its C entry; (params, exp_avg, exp_avg_sq) after every step, each checked against the restatement."""
    params = _split(case.params, case.M, case.F)
    m, v = torch.from_numpy(case.exp_avg.copy()).to(DEV), torch.from_numpy(case.exp_avg_sq.copy()).to(DEV)
    want = A.run(case)
    out = []
    for i, s in enumerate(case.steps):
        _call_entry(case, s, params, m, v)
        out.append((_join(params), m.cpu().numpy(), v.cpu().numpy()))
        _assert_same(f"{case.name}, step {i + 1}", out[-1], want[i])
    return out


def _run_fused(case):
    """The case through frame_shard.FusedAdam.step (rows=..., row masks on the buckets, its own step counts)."""
    from online_lang_splatting_amd.frame_shard import FusedAdam, GradientBucket, GradLayout
    lay = GradLayout(case.M, case.F)
    params = _split(case.params, case.M, case.F)
    adam = FusedAdam(case.P, lay, DEV)
    adam.exp_avg.copy_(torch.from_numpy(case.exp_avg))
    adam.exp_avg_sq.copy_(torch.from_numpy(case.exp_avg_sq))
    adam.step_count = case.steps[0].step - 1
    adam.group_steps = [case.steps[0].step - 1] * 7
    lrs = dict(zip(("xyz", "sh_dc", "sh_rest", "opacity", "scale", "rotation", "language"), case.lrs))
    if case.lrs[6] == 0.0:
        del lrs["language"]              # FusedAdam's default for a map without a language rate
    want = A.run(case)
    out = []
    for i, s in enumerate(case.steps):
        buckets = []
        for b, flat in enumerate(s.buckets):
            words = s.masks[b] if s.masks is not None else None
            bk = GradientBucket(case.P, lay, DEV, track_rows=words is not None)
            bk.flat.copy_(torch.from_numpy(flat))
            if words is not None:
                bk.row_mask.copy_(_mask_tensor(words))
            buckets.append(bk)
        adam.step(buckets if len(buckets) > 1 else buckets[0], params, lrs, rows=s.rows)
        torch.cuda.synchronize()
        assert adam.group_steps == [s.step] * 7
        out.append((_join(params), adam.exp_avg.cpu().numpy(), adam.exp_avg_sq.cpu().numpy()))
        _assert_same(f"{case.name}, step {i + 1}", out[-1], want[i])
    return out


@pytest.mark.parametrize("entry", A.ENTRIES)
@pytest.mark.parametrize("P,M,F", A.SHAPES)
def test_shapes(hip, P, M, F, entry):
    """Every entry at every shape: one Gaussian, a block less / exactly / more than one row, no SH (NULL), no language (NULL),
    every F the library takes, SH up to degree 3, many blocks; masked buckets hold NaN in the rows their mask clears."""
    _run_entries(A.shape_case(P, M, F, entry))


@pytest.mark.parametrize("regime", [r for r in A.REGIMES if r != "inf_and_nan"])
def test_gradient_regimes(hip, regime):
    case = A.regime_case(regime)
    out = _run_entries(case)
    if regime == "zero_rows":           # zero gradient on zero moments: p + neg_step * (0 / eps) keeps p's bits, -0.0 and +0.0 too
        for p, m, v in out:
            assert A.same_bits(p[::3], case.params[::3]).all() and not m[::3].any() and not v[::3].any()
    if regime == "square_overflows":    # v = inf, m / inf = 0: no update
        big = np.abs(case.steps[0].buckets[0]) > 1e20
        assert np.isinf(out[0][2][big]).all() and A.same_bits(out[0][0][big], case.params[big]).all()


def test_inf_and_nan_stay_in_their_element(hip):
    """One +inf and one NaN gradient element in step 2: that element's parameter goes NaN and its moments inf / NaN; every other
    element is that of the run without them."""
    with_, without = _run_entries(A.regime_case("inf_and_nan")), _run_entries(A.regime_case("inf_and_nan", special=False))
    other = np.ones(with_[0][0].shape, dtype=bool)
    for r, c, _ in A.SPECIAL:
        other[r, c] = False
    for i, (a, b) in enumerate(zip(with_, without)):
        for x, y in zip(a, b):
            assert A.same_bits(x[other], y[other]).all()
        if i >= 1:
            for r, c, _ in A.SPECIAL:
                assert np.isnan(a[0][r, c]) and not np.isfinite(a[1][r, c]) and not np.isfinite(a[2][r, c])


@pytest.mark.parametrize("step", A.STEP_COUNTS)
def test_step_counts(hip, step):
    """The bias corrections at counts 1 to 10^7 (two steps each: step and step + 1), from moments of a plausible size."""
    _run_entries(A.count_case(step))


@pytest.mark.parametrize("skip", list(A.SKIPS))
def test_group_steps_and_skips(hip, skip):
    """olsr_adam_step_groups at per-group counts (1, 2, 3, 50, 1000, 100000, 7): a skipped group keeps its parameters and moments
    bit for bit, and its gradient columns — NaN here — reach nothing that is written."""
    case = A.groups_case(skip)
    out = _run_entries(case)
    skipped = np.isin(A.column_groups(case.M, case.F), list(A.SKIPS[skip]))
    for p, m, v in out:
        assert A.same_bits(p[:, skipped], case.params[:, skipped]).all()
        assert A.same_bits(m[:, skipped], case.exp_avg[:, skipped]).all() and A.same_bits(v[:, skipped], case.exp_avg_sq[:, skipped]).all()
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()


@pytest.mark.parametrize("n", A.N_BUCKETS)
def test_several_buckets_are_summed_in_list_order(hip, n):
    """2, 3 and 8 buckets whose float32 sum depends on the order (the reverse order differs on every element for 3 and 8:
    tests/test_adam_ref_cpu.py)."""
    _run_entries(A.buckets_case(n))


@pytest.mark.parametrize("entry", ["masked", "groups"])
def test_row_masks(hip, entry):
    """Three buckets, the middle one with a NULL mask; clear bits in the first, a middle and the partial last mask word; the
    rows a mask clears hold NaN and count as +0.0."""
    out = _run_entries(A.masks_case(entry))
    assert all(np.isfinite(x).all() for step in out for x in step)


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("r0,r1", A.ROW_RANGES)
def test_row_ranges_through_fused_adam(hip, r0, r1, with_masks):
    """FusedAdam.step(rows=(r0, r1)): the pointer offsets of frame_shard.py.  Rows outside the range keep the bits of their
    pattern in parameters and both moments.  With row masks on the buckets a range that starts on a mask word (0, 64) takes the
    masked entry — its cleared rows hold NaN — and the others (1, 100) the unmasked one, with real zeros there."""
    case = A.rows_case(r0, r1, with_masks)
    out = _run_fused(case)
    outside = np.ones(case.P, dtype=bool)
    outside[r0:r1] = False
    for got in out:
        for x, start in zip(got, (case.params, case.exp_avg, case.exp_avg_sq)):
            assert A.same_bits(x[outside], start[outside]).all()
            assert np.isfinite(x).all()
    if r1 > r0:
        assert not A.same_bits(out[0][0][r0:r1], case.params[r0:r1]).all()


def test_language_rate_defaults_to_zero(hip):
    """lrs without "language": the language parameters keep their bits, their moments advance."""
    case = A.lr0_case()
    out = _run_fused(case)
    lang = A.column_groups(case.M, case.F) == 6
    for p, m, v in out:
        assert A.same_bits(p[:, lang], case.params[:, lang]).all()
        assert (m[:, lang] != 0).all() and (v[:, lang] != 0).all()
        assert not A.same_bits(p[:, ~lang], case.params[:, ~lang]).all()
