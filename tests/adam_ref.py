"""The fp32 restatement of torch/optim/adam.py::_single_tensor_adam that the three fused Adam steps are held to, bit for bit
(csrc/k_adam.hip, the Adam half of csrc/k_pose.hip, lang_ae_adam_kernel of csrc/k_lang_ae.hip), and the inputs of
tests/test_gpu_adam.py.  numpy only; written from torch's source:

    exp_avg.lerp_(grad, 1 - beta1)                                   m = m + (g - m) * f32(1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)     v = v * f32(beta2) + (f32(1 - beta2) * g) * g
    denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)    denom = sqrt(v) / f32(sqrt(bc2)) + f32(eps)
    param.addcdiv_(exp_avg, denom, value=-step_size)                 p = p + f32(-(lr / bc1)) * (m / denom)

with bc1 = 1 - beta1**step, bc2 = 1 - beta2**step in Python floats (double) and every scalar cast to float32 once; every
float32 operation is rounded once (no fused multiply-add), which is what numpy's float32 arithmetic does.  torch's own CPU
kernels fuse some of these multiply-adds, so torch on the CPU is NOT this sequence bit for bit (tests/test_adam_ref_cpu.py
measures by how much); a HIP kernel built with -ffp-contract=off, correctly rounded divide and sqrt and fp32 denormals is.

`variant` names a deliberate mistake (MUTANTS): tests/test_adam_ref_cpu.py shows that the inputs below tell every one of
them from the restatement, so a kernel that made that mistake would fail tests/test_gpu_adam.py."""
import functools
import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

f32 = np.float32
GROUPS = ("xyz", "sh_dc", "sh_rest", "opacity", "scale", "rotation", "language")   # bucket-column order
# seven distinct rates, no ratio of two a power of two (tests/test_adam_ref_cpu.py asserts it): no two -(lr / bc1) coincide
LRS = (1.6e-4, 2.5e-3, 1.3e-4, 0.05, 1e-3, 3e-3, 7e-4)

MUTANTS = tuple(f"swap_lr_{i}" for i in range(6)) + (
    "dc_boundary-1", "dc_boundary+1", "eps_before_div", "bc2_not_rooted", "step+1", "step-1", "v_fma", "lerp_two_products",
    "visible_rows_only", "bucket_sum_reversed", "masked_row_read", "skipped_group_decays", "rows_shifted")


def scalars(lr, step, betas, eps, variant=""):
    """The scalars of one step, formed in double and cast once: (1 - beta1, beta2, 1 - beta2, sqrt(bc2), eps, -(lr / bc1))."""
    beta1, beta2 = betas
    if variant == "step+1":
        step = step + 1
    elif variant == "step-1":
        step = max(step - 1, 1)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    bc2_sqrt = bc2 if variant == "bc2_not_rooted" else math.sqrt(bc2)
    return f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(bc2_sqrt), f32(eps), f32(-(lr / bc1))


def elementwise(p, m, v, g, neg_step, bc2_sqrt, betas, eps, variant=""):
    """One step on float32 arrays; neg_step and bc2_sqrt are float32 scalars or arrays that broadcast.  New (p, m, v)."""
    omb1, b2, omb2, eps = f32(1.0 - betas[0]), f32(betas[1]), f32(1.0 - betas[1]), f32(eps)
    assert all(a.dtype == f32 for a in (p, m, v, g)) and np.asarray(neg_step).dtype == f32 and np.asarray(bc2_sqrt).dtype == f32
    with np.errstate(all="ignore"):
        if variant == "lerp_two_products":
            m = m * f32(betas[0]) + g * omb1
        else:
            m = m + (g - m) * omb1
        gg = (omb2 * g) * g
        if variant == "v_fma":   # fma(v, beta2, gg): the product is exact in double, one rounding to float32
            v = (v.astype(np.float64) * np.float64(b2) + gg.astype(np.float64)).astype(f32)
        else:
            v = v * b2 + gg
        if variant == "eps_before_div":
            denom = (np.sqrt(v) + eps) / bc2_sqrt
        else:
            denom = np.sqrt(v) / bc2_sqrt + eps
        p = p + neg_step * (m / denom)
    assert p.dtype == f32 and m.dtype == f32 and v.dtype == f32
    return p, m, v


def vector_step(p, m, v, g, lr, step, betas=(0.9, 0.999), eps=1e-8, variant=""):
    """A flat parameter vector (the codec's 2 351 parameters): torch.optim.Adam's defaults."""
    _, _, _, bc2_sqrt, _, neg_step = scalars(lr, step, betas, eps, variant)
    return elementwise(p, m, v, g, neg_step, bc2_sqrt, betas, eps, variant)


def pose_step_adam(state, grad_tau, grad_exposure, lrs, step, betas=(0.9, 0.999), eps=1e-8):
    """The Adam half of olsr_pose_step on the 80-float pose state (include/olsr.h): lrs = (rot, trans, exposure);
    grad_tau = [rho | theta], rho the gradient of the translation increment.  The increments were reset to zero by the last
    update_pose, so tau = 0 + neg_step * (m / denom).  grad_exposure None: the exposure pair does not step.
    Returns dict(tau, tau_m, tau_v, exposure, exposure_m, exposure_v)."""
    state = np.asarray(state, dtype=f32)
    lr_rot, lr_trans, lr_exposure = lrs
    _, _, _, bc2_sqrt, _, neg_rot = scalars(lr_rot, step, betas, eps)
    neg_trans, neg_exposure = scalars(lr_trans, step, betas, eps)[5], scalars(lr_exposure, step, betas, eps)[5]
    neg = np.array([neg_trans] * 3 + [neg_rot] * 3, dtype=f32)
    tau, tm, tv = elementwise(np.zeros(6, f32), state[52:58], state[58:64], np.asarray(grad_tau, dtype=f32), neg, bc2_sqrt, betas, eps)
    out = dict(tau=tau, tau_m=tm, tau_v=tv, exposure=state[70:72].copy(), exposure_m=state[72:74].copy(),
               exposure_v=state[74:76].copy())
    if grad_exposure is not None:
        out["exposure"], out["exposure_m"], out["exposure_v"] = elementwise(
            state[70:72], state[72:74], state[74:76], np.asarray(grad_exposure, dtype=f32), neg_exposure, bc2_sqrt, betas, eps)
    return out


# ---- the Gaussian map's step over the bucket row layout ----------------------------------------------------------------------
def width_of(M, F):
    return 11 + 3 * M + F


def column_groups(M, F, dc_shift=0):
    """Group index (GROUPS) of every column of [3 xyz | 3M sh | 1 opacity | 3 scale | 4 rotation | F language]; sh_dc is the
    first three SH columns (columns 3..5)."""
    sh = [1 if c < 3 + dc_shift else 2 for c in range(3 * M)]
    return np.array([0] * 3 + sh + [3] + [4] * 3 + [5] * 4 + [6] * F, dtype=np.int64)


def mask_bits(mask, P):
    """uint64 words -> bool[P]: bit g % 64 of word g // 64 (set = the row is read)."""
    if mask is None:
        return np.ones(P, dtype=bool)
    rows = np.arange(P)
    return ((np.asarray(mask, dtype=np.uint64)[rows // 64] >> (rows % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def bucket_sum(buckets, masks, variant=""):
    """((f0 + f1) + f2) + ... in float32; a row that a bucket's mask clears contributes +0.0 whatever the bucket holds."""
    P = buckets[0].shape[0]
    masks = list(masks) if masks is not None else [None] * len(buckets)
    pairs = list(zip(buckets, masks))
    if variant == "bucket_sum_reversed":
        pairs = pairs[::-1]
    total = None
    with np.errstate(all="ignore"):
        for flat, mask in pairs:
            assert flat.dtype == f32
            bits = np.ones(P, dtype=bool) if variant == "masked_row_read" else mask_bits(mask, P)
            term = np.where(bits[:, None], flat, f32(0.0))
            total = term if total is None else total + term
    return total


def gaussian_step(params, exp_avg, exp_avg_sq, buckets, masks, lrs, M, F, step=None, group_steps=None, skip=(), rows=None,
                  betas=(0.9, 0.999), eps=1e-15, variant=""):
    """One step of the map's optimiser on [P, width] float32 arrays in the bucket's column layout.  step: one count for every
    group, or group_steps: the count each group steps at; skip: indices of groups that do not step (parameters and moments
    untouched); rows = (r0, r1): only those rows change.  Returns new (params, exp_avg, exp_avg_sq)."""
    P, width = params.shape
    assert width == width_of(M, F) and (step is None) != (group_steps is None)
    lrs = list(lrs)
    if variant.startswith("swap_lr_"):
        i = int(variant[-1])
        lrs[i], lrs[i + 1] = lrs[i + 1], lrs[i]
    grp = column_groups(M, F, {"dc_boundary-1": -1, "dc_boundary+1": 1}.get(variant, 0))
    steps = [step] * 7 if group_steps is None else list(group_steps)
    per_group = [scalars(lrs[g], max(int(steps[g]), 1), betas, eps, variant) for g in range(7)]
    neg_step = np.array([per_group[g][5] for g in grp], dtype=f32)
    bc2_sqrt = np.array([per_group[g][3] for g in grp], dtype=f32)
    r0, r1 = (0, P) if rows is None else rows
    if variant == "rows_shifted" and rows is not None:
        r0, r1 = min(r0 + 1, P), min(r1 + 1, P)
    g = bucket_sum(buckets, masks, variant)
    p, m, v = elementwise(params, exp_avg, exp_avg_sq, g, neg_step, bc2_sqrt, betas, eps, variant)
    change = np.zeros((P, width), dtype=bool)
    change[r0:r1] = True
    skipped = np.isin(grp, list(skip))
    change[:, skipped] = False
    if variant == "visible_rows_only":
        change[~(g != 0).any(axis=1)] = False
    p, m, v = np.where(change, p, params), np.where(change, m, exp_avg), np.where(change, v, exp_avg_sq)
    if variant == "skipped_group_decays" and skipped.any():
        with np.errstate(all="ignore"):
            zero = np.zeros_like(params)
            _, dm, dv = elementwise(params, exp_avg, exp_avg_sq, zero, neg_step, bc2_sqrt, betas, eps)
        inside = np.zeros((P, width), dtype=bool)
        inside[r0:r1, skipped] = True
        m, v = np.where(inside, dm, m), np.where(inside, dv, v)
    return p, m, v


def same_bits(a, b):
    """Elementwise: equal including the sign of zero, or both NaN."""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- the inputs of tests/test_gpu_adam.py --------------------------------------------------------------------------------------
@dataclass
class Step:
    buckets: List[np.ndarray]
    masks: Optional[List[Optional[np.ndarray]]] = None
    step: Optional[int] = None
    group_steps: Optional[List[int]] = None
    skip: Tuple[int, ...] = ()
    rows: Optional[Tuple[int, int]] = None


@dataclass
class Case:
    """entry: which C entry runs it — "step", "sum", "masked", "groups" — or "fused": frame_shard.FusedAdam.step, which keeps
    the counts itself (they are in the steps all the same: the restatement needs them)."""
    name: str
    entry: str
    P: int
    M: int
    F: int
    params: np.ndarray
    exp_avg: np.ndarray
    exp_avg_sq: np.ndarray
    steps: List[Step]
    lrs: Tuple[float, ...] = LRS
    note: dict = field(default_factory=dict)


def run(case, variant=""):
    """The restatement's (params, exp_avg, exp_avg_sq) after every step of the case."""
    p, m, v = case.params, case.exp_avg, case.exp_avg_sq
    out = []
    for s in case.steps:
        p, m, v = gaussian_step(p, m, v, s.buckets, s.masks, case.lrs, case.M, case.F, step=s.step, group_steps=s.group_steps,
                                skip=s.skip, rows=s.rows, variant=variant)
        out.append((p, m, v))
    return out


def _rng(*key):
    return np.random.default_rng([20261018, *key])


def mixed_params(rng, P, M, F, lrs=LRS):
    """A third O(1), a third of a magnitude at or below one step of their group (a step of Adam is about lr), a third exact
    zeros: the displacement's own bits show instead of drowning in the rounding of an O(1) parameter."""
    w = width_of(M, F)
    lr = np.array([lrs[g] for g in column_groups(M, F)], dtype=np.float64)
    kind = rng.integers(0, 3, size=(P, w))
    big = rng.standard_normal((P, w))
    small = rng.uniform(-1.0, 1.0, size=(P, w)) * lr
    return np.where(kind == 0, big, np.where(kind == 1, small, 0.0)).astype(f32)


def moments(rng, P, w, scale=1e-3):
    """Moments of a plausible size for gradients of `scale`."""
    return (rng.standard_normal((P, w)) * scale).astype(f32), (rng.uniform(0.0, 1.0, size=(P, w)) * scale * scale).astype(f32)


def ordinary(rng, P, w, scale=1e-3):
    return (rng.standard_normal((P, w)) * scale).astype(f32)


def log_uniform(rng, P, w, lo, hi):
    """|g| log-uniform in [lo, hi], random sign."""
    mag = np.exp(rng.uniform(math.log(lo), math.log(hi), size=(P, w)))
    return (mag * rng.choice([-1.0, 1.0], size=(P, w))).astype(f32)


def random_mask(rng, P, clear_in=None):
    """uint64 row-mask words for P rows, about half the bits clear; clear_in: rows that must be clear."""
    bits = rng.random(P) < 0.5
    if clear_in is not None:
        bits[list(clear_in)] = False
    words = np.zeros((P + 63) // 64, dtype=np.uint64)
    for r in np.nonzero(bits)[0]:
        words[r // 64] |= np.uint64(1) << np.uint64(r % 64)
    return words


def poison_cleared(flat, mask, value=np.nan):
    """The rows a mask clears hold `value` in the bucket: a kernel that read them would show it."""
    out = flat.copy()
    out[~mask_bits(mask, flat.shape[0])] = value
    return out


SHAPES = ((1, 1, 0), (63, 0, 0), (64, 1, 15), (65, 4, 3), (129, 16, 32), (4097, 2, 16), (130, 0, 32))
ENTRIES = ("step", "sum", "masked", "groups")
GROUP_LAG = (3, 1, 2, 5, 1, 4, 2)            # the shape cases' per-group counts at their first step
REGIMES = ("ordinary", "zero_rows", "eps_dominated", "square_overflows", "inf_and_nan", "denormal_products")
STEP_COUNTS = (1, 2, 10, 1000, 100000, 10_000_000)
GROUP_STEP = (1, 2, 3, 50, 1000, 100000, 7)
SKIPS = {"none": (), "opacity": (3,), "all_but_language": (0, 1, 2, 3, 4, 5), "xyz_rotation": (0, 5)}
N_BUCKETS = (2, 3, 8)
ROW_RANGES = ((0, 64), (1, 65), (64, 130), (100, 101), (37, 37))
RP, RM, RF = 130, 2, 15                       # the shape of the regime, count, bucket, mask and row-range cases
SPECIAL = ((5, 2, np.inf), (77, 20, np.nan))  # (row, column, value) of the inf_and_nan regime


@functools.lru_cache(maxsize=None)
def shape_case(P, M, F, entry):
    rng = _rng(1, P, M, F, ENTRIES.index(entry))
    w = width_of(M, F)
    steps = []
    for i in range(3):
        if entry == "step":
            steps.append(Step([ordinary(rng, P, w)], step=i + 1))
        elif entry == "sum":
            steps.append(Step([ordinary(rng, P, w), ordinary(rng, P, w)], step=i + 1))
        else:
            masks = [random_mask(rng, P), None]
            buckets = [poison_cleared(ordinary(rng, P, w), masks[0]), ordinary(rng, P, w)]
            if entry == "masked":
                steps.append(Step(buckets, masks, step=i + 1))
            else:
                steps.append(Step(buckets, masks, group_steps=[s + i for s in GROUP_LAG]))
    m, v = (np.zeros((P, w), f32), np.zeros((P, w), f32)) if entry in ("step", "sum", "masked") else moments(rng, P, w)
    return Case(f"shape P={P} M={M} F={F} {entry}", entry, P, M, F, mixed_params(rng, P, M, F), m, v, steps)


@functools.lru_cache(maxsize=None)
def regime_case(regime, special=True):
    """Three steps at P=130, M=2, F=15 through olsr_adam_step.  special=False (inf_and_nan only): the same run without the
    two special elements."""
    rng = _rng(2)   # the same draws for every regime: the inf_and_nan run is the ordinary run but for two elements
    P, M, F = RP, RM, RF
    w = width_of(M, F)
    params = mixed_params(rng, P, M, F)
    steps = []
    for i in range(3):
        g = ordinary(rng, P, w)
        if regime == "ordinary" and i == 1:
            g[1::3] = 0.0                    # zero gradient on moments that are not zero: the rows still move (dense Adam)
        elif regime == "zero_rows":
            g[::3] = 0.0                     # zero from step 1 on, zero moments: the rows must not change at all
        elif regime == "eps_dominated":
            g = log_uniform(rng, P, w, 1e-17, 1e-13)
        elif regime == "square_overflows":
            g = (rng.choice([-1.0, 1.0], size=(P, w)) * 1e25).astype(f32)
            g[::2] = ordinary(rng, P, w)[::2]
        elif regime == "inf_and_nan" and special and i == 1:
            for r, c, val in SPECIAL:
                g[r, c] = val
        elif regime == "denormal_products":
            g = log_uniform(rng, P, w, 1e-23, 1e-19)
        steps.append(Step([g], step=i + 1))
    z = np.zeros((P, w), f32)
    return Case(f"regime {regime}" + ("" if special else " without the special elements"), "step", P, M, F, params, z, z.copy(), steps)


@functools.lru_cache(maxsize=None)
def count_case(step):
    rng = _rng(3, step)
    w = width_of(RM, RF)
    m, v = moments(rng, RP, w)
    steps = [Step([ordinary(rng, RP, w)], step=step), Step([ordinary(rng, RP, w)], step=step + 1)]
    return Case(f"step count {step}", "step", RP, RM, RF, mixed_params(rng, RP, RM, RF), m, v, steps)


@functools.lru_cache(maxsize=None)
def groups_case(skip_name):
    """group_step = GROUP_STEP with a skip mask; the gradient columns of skipped groups are NaN."""
    rng = _rng(4, sorted(SKIPS).index(skip_name))
    skip = SKIPS[skip_name]
    w = width_of(RM, RF)
    m, v = moments(rng, RP, w)
    skipped = np.isin(column_groups(RM, RF), list(skip))
    steps = []
    for i in range(2):
        g = ordinary(rng, RP, w)
        g[:, skipped] = np.nan
        steps.append(Step([g], None, group_steps=[s + (0 if gi in skip else i) for gi, s in enumerate(GROUP_STEP)], skip=skip))
    return Case(f"groups skip {skip_name}", "groups", RP, RM, RF, mixed_params(rng, RP, RM, RF), m, v, steps)


def order_dependent_buckets(rng, n, P, w):
    """n buckets whose float32 sum depends on the order: a value, then its near-negative (their sum is exact, about 1e-6 of
    the value), then values six to nine decades below the first.  In list order the small ones meet a small partial sum and
    keep their bits; in reverse they are added to the large value first and lose them."""
    x = ordinary(rng, P, w)
    out = [x, (-x.astype(np.float64) * (1.0 + rng.uniform(-1e-6, 1e-6, size=(P, w)))).astype(f32)]
    for _ in range(n - 2):
        out.append((x.astype(np.float64) * rng.choice([-1.0, 1.0], size=(P, w)) * 10.0 ** rng.uniform(-9.0, -6.0, size=(P, w))).astype(f32))
    return out


@functools.lru_cache(maxsize=None)
def buckets_case(n):
    rng = _rng(5, n)
    w = width_of(RM, RF)
    m, v = moments(rng, RP, w, 1e-9)
    steps = [Step(order_dependent_buckets(rng, n, RP, w), step=4 + i) for i in range(2)]
    return Case(f"{n} buckets", "sum", RP, RM, RF, mixed_params(rng, RP, RM, RF), m, v, steps)


def _three_masked_buckets(rng, P, w, poison):
    """Three buckets, the middle one without a mask; the others' masks clear rows in the first, the middle and the partial
    last word (P = 130: rows 0..63, 64..127, 128..129)."""
    masks = [random_mask(rng, P, clear_in=(3, 70, 129)), None, random_mask(rng, P, clear_in=(60, 100, 128))]
    buckets = [ordinary(rng, P, w) for _ in range(3)]
    for b in (0, 2):
        buckets[b] = poison_cleared(buckets[b], masks[b], poison)
    return buckets, masks


@functools.lru_cache(maxsize=None)
def masks_case(entry):
    rng = _rng(6, ENTRIES.index(entry))
    w = width_of(RM, RF)
    m, v = moments(rng, RP, w)
    steps = []
    for i in range(2):
        buckets, masks = _three_masked_buckets(rng, RP, w, np.nan)
        steps.append(Step(buckets, masks, step=7 + i) if entry == "masked" else
                     Step(buckets, masks, group_steps=[s + i for s in GROUP_LAG]))
    return Case(f"masks {entry}", entry, RP, RM, RF, mixed_params(rng, RP, RM, RF), m, v, steps)


@functools.lru_cache(maxsize=None)
def rows_case(r0, r1, with_masks):
    """FusedAdam.step(rows=(r0, r1)), two steps at counts 5 and 6.  The parameters and moments are a recognisable pattern
    (row + column / 128, scaled) so that a row written outside the range shows.  With row masks the cleared rows hold NaN
    where the range starts on a mask word (the masked entry) and real zeros where it does not (the unmasked one)."""
    rng = _rng(7, r0, r1, int(with_masks))
    P, w = RP, width_of(RM, RF)
    pattern = (np.arange(P)[:, None] + np.arange(w)[None, :] / 128.0).astype(f32)
    params = (pattern * f32(2.0 ** -7)).astype(f32)
    m, v = (pattern * f32(1e-5)).astype(f32), (pattern * f32(1e-9) + f32(1e-9)).astype(f32)
    steps = []
    for i in range(2):
        if with_masks:
            buckets, masks = _three_masked_buckets(rng, P, w, np.nan if r0 % 64 == 0 else 0.0)
        else:
            buckets, masks = [ordinary(rng, P, w)], None
        steps.append(Step(buckets, masks, step=5 + i, rows=(r0, r1)))
    return Case(f"rows ({r0}, {r1})" + (" with row masks" if with_masks else ""), "fused", P, RM, RF, params, m, v, steps)


@functools.lru_cache(maxsize=None)
def lr0_case():
    """No "language" rate given: FusedAdam's lrs.get("language", 0.0).  The language parameters keep their bits (p + -0.0 * x),
    their moments advance."""
    rng = _rng(8)
    w = width_of(RM, RF)
    steps = [Step([ordinary(rng, RP, w)], step=i + 1) for i in range(2)]
    z = np.zeros((RP, w), f32)
    return Case("language rate 0", "fused", RP, RM, RF, mixed_params(rng, RP, RM, RF), z, z.copy(), steps, lrs=LRS[:6] + (0.0,))


def all_cases():
    """Every case of tests/test_gpu_adam.py, in its order."""
    out = [shape_case(P, M, F, e) for (P, M, F) in SHAPES for e in ENTRIES]
    out += [regime_case(r) for r in REGIMES]
    out += [count_case(s) for s in STEP_COUNTS]
    out += [groups_case(k) for k in SKIPS]
    out += [buckets_case(n) for n in N_BUCKETS]
    out += [masks_case(e) for e in ("masked", "groups")]
    out += [rows_case(r0, r1, wm) for (r0, r1) in ROW_RANGES for wm in (False, True)]
    out.append(lr0_case())
    return out
