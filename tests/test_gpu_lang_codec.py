"""olsr_lang_ae_train_step / _encode / _decode (HIP), lang_codec.OnlineLanguageCodec and slam_iterations.OnlineLanguageTargets
on the GPU.

Yardstick: the project's own, from tests/test_gpu_ssim.py — the reference's float32 error, not a tolerance chosen in
advance.  With `truth` the float64 and `ref32` the float32 evaluation of the reference's statements (tests/golden/
lang_codec.npz for the gradient and the losses; tests/lang_codec_ref.py, which tests/test_lang_codec_ref_golden.py pins to that
file, for per-row codes and the full sizes), err_hip = |hip - truth|, err_ref = |ref32 - truth|:
    per gradient tensor, and the codes   max(err_hip) <= max(4 max(err_ref), 4 * 2^-24 max|truth|), and the same for rms
    scalars                              |hip - truth| <= max(4 |ref32 - truth|, 4 * 2^-24)
4x: another summation order of the same float32 products has errors of the same size (measured on the CPU when the cases
were designed: a row permutation and 256-row partials added in double gave a worst ratio of 1.8 against ref32 over the eight
golden cases); 4 * 2^-24 is two ulp of a float32 of magnitude 1.  The single-step cases are free of tie rows
(tests/lang_codec_ref.py), whose one-sided rounding no summation order can follow.  Every figure is printed.
"""
import pytest
import torch

import adam_ref
import lang_codec_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP2 = 4.0 * 2.0 ** -24


def _rms(e):
    return float(torch.sqrt((e.double() ** 2).mean()))


def _ratio_rule(label, hip, truth, ref32):
    truth = truth.double()
    e_hip, e_ref = (hip.double() - truth).abs(), (ref32.double() - truth).abs()
    floor = ULP2 * float(truth.abs().max())
    mx, rm = (float(e_hip.max()), float(e_ref.max())), (_rms(e_hip), _rms(e_ref))
    print(f"{label}: scale {float(truth.abs().max()):.3e}; max error hip {mx[0]:.3e} ref {mx[1]:.3e} "
          f"(ratio {mx[0] / mx[1] if mx[1] > 0 else float('nan'):.3g}); rms hip {rm[0]:.3e} ref {rm[1]:.3e} "
          f"(ratio {rm[0] / rm[1] if rm[1] > 0 else float('nan'):.3g})")
    assert torch.isfinite(hip).all(), label
    assert mx[0] <= max(4.0 * mx[1], floor), (label, "max", mx, floor)
    assert rm[0] <= max(4.0 * rm[1], floor), (label, "rms", rm, floor)


def _scalar_rule(label, hip, truth, ref32):
    e_hip, e_ref = abs(float(hip) - float(truth)), abs(float(ref32) - float(truth))
    print(f"{label}: hip {float(hip):.9g} truth {float(truth):.9g}; error hip {e_hip:.3e} ref {e_ref:.3e}")
    assert e_hip <= max(4.0 * e_ref, ULP2), (label, e_hip, e_ref)


def _codec(flat):
    from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec
    c = OnlineLanguageCodec(DEV, seed=0)
    c.load_state_dict(R.unflatten(flat))
    assert torch.equal(c.flat.cpu(), flat)
    return c


LOSS_NAMES = ("total", "L1", "0.6 (1 - cos)", "mean cos")


def _check_step0(label, flat, x, truth, ref32):
    """truth / ref32: dict(loss [>=1,4], grad0, codes_pre0) on the CPU."""
    xd = x.to(DEV)
    c = _codec(flat)
    grad = torch.full((R.N_PARAMS,), float("nan"), device=DEV)
    loss, codes = c.train_step(xd, 1e-3, codes="pre", layout="rows", grad_out=grad)
    loss, codes, grad = loss.cpu(), codes.cpu().clone(), grad.cpu()
    for (name, _), g_hip, g_t, g_r in zip(R.STATE, R.unflatten(grad).values(), R.unflatten(truth["grad0"]).values(),
                                          R.unflatten(ref32["grad0"]).values()):
        _ratio_rule(f"{label} d {name}", g_hip, g_t, g_r)
    for k, name in enumerate(LOSS_NAMES):
        _scalar_rule(f"{label} {name}", loss[k], truth["loss"][0, k], ref32["loss"][0, k])
    _ratio_rule(f"{label} codes", codes, truth["codes_pre0"], ref32["codes_pre0"])
    # the channel-major layout: the same codes, transposed, bit for bit; same loss and gradient
    c2 = _codec(flat)
    grad2 = torch.zeros(R.N_PARAMS, device=DEV)
    loss2, codes2 = c2.train_step(xd, 1e-3, codes="pre", layout="channels", grad_out=grad2)
    assert tuple(codes2.shape) == (15, x.shape[0])
    assert torch.equal(codes2.cpu(), codes.t()) and torch.equal(loss2.cpu(), loss) and torch.equal(grad2.cpu(), grad)
    assert torch.equal(c2.flat, c.flat) and int(c.step_dev) == 1
    return c, grad


def _golden_case(key):
    z = R.golden()
    flat, x = torch.from_numpy(z[f"{key}_params"]), R.unit(z[f"{key}_q"])
    lr, steps = float(z["lr"]), int(z["steps"])
    t64, t32 = R.train(flat, x, lr, steps, torch.float64), R.train(flat, x, lr, steps, torch.float32)
    # the gradient and the losses are the recorded ones, not the restatement's
    for t, tag in ((t64, "f64"), (t32, "f32")):
        t["grad0"] = torch.from_numpy(z[f"{key}_grad0_{tag}"])
        t["loss"] = torch.from_numpy(z[f"{key}_loss_{tag}"])
    return flat, x, lr, steps, t64, t32


@pytest.mark.parametrize("key,N,seed", R.golden_cases())
def test_step0_golden(hip, key, N, seed):
    flat, x, _, _, t64, t32 = _golden_case(key)
    _check_step0(f"golden {key}", flat, x, t64, t32)


@pytest.mark.parametrize("N,seed", [(36864, 0), (36865, 1)])
def test_step0_full_size(hip, N, seed):
    flat, q, redrawn = R.make_case(N, seed)
    print(f"N = {N}: {redrawn} rows redrawn by the tie filter")
    x = R.unit(q)
    _check_step0(f"full size {N}", flat, x, R.train(flat, x, 1e-3, 1, torch.float64), R.train(flat, x, 1e-3, 1, torch.float32))


def _assert_adam(c, p, opt):
    """The criterion of tests/test_gpu_api.py::test_fused_adam_equals_torch_optim_adam: parameters rtol 2e-6 / atol 2e-7 (one ulp of an
    O(1) parameter), exp_avg rtol 1e-5 / atol 2e-9, exp_avg_sq rtol 1e-5 / atol 1e-11."""
    st = opt.state[p]
    d = float((c.flat.cpu() - p.detach()).abs().max())
    torch.testing.assert_close(c.flat.cpu(), p.detach(), rtol=2e-6, atol=2e-7)
    torch.testing.assert_close(c.exp_avg.cpu(), st["exp_avg"], rtol=1e-5, atol=2e-9)
    torch.testing.assert_close(c.exp_avg_sq.cpu(), st["exp_avg_sq"], rtol=1e-5, atol=1e-11)
    return d


@pytest.mark.parametrize("key", ["n1000_s0", "n257_s3"])
@pytest.mark.parametrize("counter", ["device", "caller"])
def test_adam_on_the_recorded_gradient(hip, key, counter):
    """The parameters and moments after every one of six steps are torch.optim.Adam's on the float32 gradient that step
    recorded (grad_out), to the criterion the fused bucket Adam is held to.  counter = "device": the step count is the device
    word alone (step = 0 in every call); "caller": the caller passes 1, 2, ... (the device word still counts the calls)."""
    flat, x, lr, _, _, _ = _golden_case(key)
    xd = x.to(DEV)
    c = _codec(flat)
    p = flat.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    for i in range(6):
        grad = torch.zeros(R.N_PARAMS, device=DEV)
        c.train_step(xd, lr, codes=None, grad_out=grad, step=0 if counter == "device" else i + 1)
        p.grad = grad.cpu()
        opt.step()
        d = _assert_adam(c, p, opt)
        moved = float((c.flat.cpu() - flat).abs().max())
        print(f"{key} {counter} counter, step {i + 1}: largest parameter move {moved:.3e}, largest distance to torch.optim.Adam {d:.3e}")
        assert moved > 0.5 * lr
        assert int(c.step_dev) == i + 1


@pytest.mark.parametrize("key", ["n1000_s0", "n257_s3"])
def test_adam_on_the_recorded_gradient_equals_the_fp32_restatement(hip, key):
    """lang_ae_adam_kernel with the caller's counter: the 2 351 parameters and both moments after each of six steps equal, bit
    for bit (a == b or both NaN, the sign of zero included), adam_ref.vector_step — the unfused float32 sequence of torch's
    single-tensor Adam — applied to the float32 gradient that step recorded (grad_out)."""
    flat, x, lr, _, _, _ = _golden_case(key)
    xd = x.to(DEV)
    c = _codec(flat)
    p, m, v = flat.numpy().copy(), c.exp_avg.cpu().numpy().copy(), c.exp_avg_sq.cpu().numpy().copy()
    assert not m.any() and not v.any()
    for i in range(6):
        grad = torch.zeros(R.N_PARAMS, device=DEV)
        c.train_step(xd, lr, codes=None, grad_out=grad, step=i + 1)
        p, m, v = adam_ref.vector_step(p, m, v, grad.cpu().numpy(), lr, i + 1)
        for name, got, want in (("parameters", c.flat, p), ("exp_avg", c.exp_avg, m), ("exp_avg_sq", c.exp_avg_sq, v)):
            same = adam_ref.same_bits(got.cpu().numpy(), want)
            assert same.all(), (key, i + 1, name, int((~same).sum()))


@pytest.mark.parametrize("key,N,seed", R.golden_cases())
def test_training_30_steps(hip, key, N, seed):
    """30 steps enqueued without a synchronisation, the step count on the device."""
    flat, x, lr, steps, t64, t32 = _golden_case(key)
    xd = x.to(DEV)
    c = _codec(flat)
    losses = torch.empty(steps, 4, device=DEV)
    codes = None
    for i in range(steps):
        loss, codes = c.train_step(xd, lr, codes="post" if i == steps - 1 else None)
        losses[i].copy_(loss)
    losses, codes = losses.cpu(), codes.cpu()
    assert int(c.step_dev) == steps
    worst = 0.0
    for i in range(steps):
        for k in range(4):
            e_hip, e_ref = abs(float(losses[i, k]) - float(t64["loss"][i, k])), abs(float(t32["loss"][i, k]) - float(t64["loss"][i, k]))
            worst = max(worst, e_hip)
            assert e_hip <= max(4.0 * e_ref, ULP2), (key, i, LOSS_NAMES[k], e_hip, e_ref)
    e_ref_last = abs(float(t32["loss"][-1, 0]) - float(t64["loss"][-1, 0]))
    print(f"{key}: loss {float(losses[0, 0]):.6f} -> {float(losses[-1, 0]):.6f}; largest loss-term error over {steps} steps "
          f"{worst:.3e} (ref32, total loss of the last step: {e_ref_last:.3e})")
    _ratio_rule(f"{key} codes after {steps} steps", codes, t64["codes_post"], t32["codes_post"])
    e = (c.flat.cpu().double() - t64["params"]).abs().max()
    print(f"{key}: parameters after {steps} steps: max error hip {float(e):.3e} ref "
          f"{float((t32['params'].double() - t64['params']).abs().max()):.3e}")


def test_encode_decode_are_the_train_steps_path(hip):
    flat, x, lr, _, t64, t32 = _golden_case("n1000_s2")
    xd = x.to(DEV)
    c = _codec(flat)
    enc = c.encode(xd).clone()
    enc_t = c.encode(xd, "channels").clone()
    rec = c.decode(enc).clone()
    assert torch.equal(enc_t, enc.t()) and torch.equal(c.decode(enc_t, "channels"), rec)
    loss, pre = c.train_step(xd, lr, codes="pre")
    assert torch.equal(pre, enc)                                              # the train step's codes, bit for bit
    # its reconstruction: the loss terms evaluated on decode's output in float64 are the step's
    r, xx = rec.double().cpu(), x.double()
    l1 = (r - xx).abs().mean()
    cos = torch.nn.functional.cosine_similarity(r, xx, dim=1).mean()
    for k, v in enumerate((l1 + 0.6 * (1 - cos), l1, 0.6 * (1 - cos), cos)):
        assert abs(float(loss[k]) - float(v)) <= ULP2, (k, float(loss[k]), float(v))
    # unit norms
    n_rec, n_enc = rec.double().norm(dim=1), enc.double().norm(dim=1)
    print(f"largest | |decode| - 1 | {float((n_rec - 1).abs().max()):.3e}, | |encode| - 1 | {float((n_enc - 1).abs().max()):.3e}")
    assert float((n_rec - 1).abs().max()) <= ULP2 and float((n_enc - 1).abs().max()) <= ULP2
    _ratio_rule("decode", rec.cpu(), R.codec_from(flat, torch.float64).decode(t64["codes_pre0"]).detach(),
                R.codec_from(flat, torch.float32).decode(t32["codes_pre0"]).detach())
    # "post": the codes of the updated parameters, one more launch
    _, post = c.train_step(xd, lr, codes="post")
    assert torch.equal(post, c.encode(xd)) and not torch.equal(post, enc)
    # language_target: [15,h,w] = codes.T.view(15, h, w)
    t = c.language_target(xd[:24 * 40], hw=(24, 40))
    assert tuple(t.shape) == (15, 24, 40) and torch.equal(t.reshape(15, -1), c.encode(xd[:24 * 40]).t())


def test_two_runs_are_bit_identical(hip):
    flat, q, _ = R.make_case(36865, 2)
    xd = R.unit(q).to(DEV)
    xd1 = torch.zeros(xd.numel() + 1, device=DEV)[1:].view_as(xd)             # an unaligned copy: the scalar loads
    xd1.copy_(xd)
    outs = []
    for feats in (xd, xd, xd1):
        c = _codec(flat)
        c._scratch = torch.full((c_scratch_bytes(xd.shape[0]),), 0xFF, dtype=torch.uint8, device=DEV)   # poisoned scratch
        c._scratch_n = xd.shape[0]
        for i in range(5):
            loss, codes = c.train_step(feats, 1e-3, codes="post" if i == 4 else "pre")
        outs.append((c.flat.clone(), c.exp_avg.clone(), c.exp_avg_sq.clone(), loss.clone(), codes.clone()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][3]).all()


def c_scratch_bytes(N):
    from online_lang_splatting_amd import _lib
    return _lib.lib().olsr_lang_ae_scratch_bytes(N)


def test_python_argument_errors(hip):
    c = _codec(R.initial_params(0))
    x = torch.rand(64, 32, device=DEV)
    with pytest.raises(RuntimeError, match="GPU"):
        c.train_step(x.cpu(), 1e-4)
    with pytest.raises(RuntimeError, match="GPU"):
        c.encode(x.double())
    with pytest.raises(RuntimeError, match=r"\[N,32\]"):
        c.encode(torch.rand(64, 31, device=DEV))
    with pytest.raises(RuntimeError, match=r"\[N,15\]"):
        c.decode(torch.rand(64, 16, device=DEV))
    with pytest.raises(RuntimeError, match=r"\[15,N\]"):
        c.decode(torch.rand(64, 15, device=DEV), "channels")
    with pytest.raises(RuntimeError, match="grad_out"):
        c.train_step(x, 1e-4, grad_out=torch.zeros(2351))
    with pytest.raises(RuntimeError, match="layout"):
        c.encode(x, "columns")
    with pytest.raises(RuntimeError, match="codes must be"):
        c.train_step(x, 1e-4, codes="both")
    with pytest.raises(RuntimeError, match="language_target"):
        c.language_target(x, hw=(192, 192))
    sd = c.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in R.STATE]
    m = R.Codec()
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})                    # a torch module of the reference's structure takes it
    c.load_state_dict(m.state_dict())


# ---- the sequencing of map() ---------------------------------------------------------------------------------------------
LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)


def test_online_language_targets(hip):
    from online_lang_splatting_amd.frame_shard import FrameLanes
    from online_lang_splatting_amd.scene import make_room_scene
    from online_lang_splatting_amd.slam_iterations import MappingStep, OnlineLanguageTargets
    dev = torch.device(DEV)
    views = 3
    g = torch.Generator().manual_seed(9)
    feats = [R.unit(R.draw_q(192 * 192, g)).to(dev) for _ in range(views)]
    c = _codec(R.initial_params(3))
    lt = OnlineLanguageTargets(c, lr=1e-4)
    for v in range(views):
        want = c.language_target(feats[v])                                    # the codes of the parameters before the step
        before = c.flat.clone()
        got = lt.add_keyframe(v, feats[v])
        assert tuple(got.shape) == (15, 192, 192) and torch.equal(got, want)
        assert not torch.equal(c.flat, before)                                # ... and the step was taken
    assert lt.steps == views and int(c.step_dev) == views
    reused = feats[0].clone()
    lt2 = OnlineLanguageTargets(_codec(R.initial_params(3)), lr=1e-4)
    lt2.add_keyframe("a", reused)
    kept, loss_a = lt2.features["a"].clone(), lt2.last_loss.clone()
    reused.zero_()                                                            # the caller reuses its buffer
    assert torch.equal(lt2.features["a"], kept) and torch.equal(kept, feats[0])
    lt2.rehearse(["a"])
    assert torch.equal(lt2.features["a"], kept) and not torch.equal(lt2.last_loss, loss_a)
    stored = [t.clone() for t in lt.targets_for(range(views))]
    before = c.flat.clone()
    lt.rehearse([2, 0])
    assert not torch.equal(c.flat, before) and lt.steps == views + 2 and int(c.step_dev) == views + 2
    for a, b in zip(stored, lt.targets_for(range(views))):
        assert torch.equal(a, b)                                              # rehearsal leaves the stored targets alone
    assert float(lt.last_loss[0]) > 0 and torch.isfinite(lt.last_loss).all()
    with pytest.raises(KeyError):
        lt.rehearse([7])
    # a mapping iteration on a small scene with those targets in the third slot
    W, H, F = 320, 184, 15
    rs = make_room_scene(12_000, W, H, F, views=views, seed=5)
    sc = rs.scene
    params = dict(means3D=sc.means3D, shs=sc.shs, opacities=torch.logit(sc.opacities), scales=torch.log(sc.scales),
                  rotations=sc.rotations, language=sc.language)
    params = {k: v.to(dev).contiguous() for k, v in params.items()}
    start = params["language"].clone()
    camd = [dict(viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
                 projmatrix_raw=cam.projection_matrix.to(dev), campos=cam.camera_center.to(dev), tanfovx=cam.tanfovx,
                 tanfovy=cam.tanfovy) for cam in rs.cameras]
    targets = [(a, b, t) for (a, b, _), t in zip(rs.targets, lt.targets_for(range(views)))]
    lanes = FrameLanes(1, sc.P, W, H, F, sc.shs.shape[1], 600_000, dev)
    ms = MappingStep(lanes, params, sc.bg.to(dev), 0, camd, targets, LRS, exposure=torch.zeros(2, device=dev), fused_loss=True)
    ms.iteration()
    lt.rehearse([1, 2])
    ms.iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(ms.last_loss).all() and float(ms.last_loss.reshape(-1, 4)[..., 3].abs().sum()) > 0   # a language term
    assert torch.isfinite(params["language"]).all() and not torch.equal(params["language"], start)


def _raises_exactly(sentence):
    """pytest.raises for a RuntimeError whose whole message is `sentence`."""
    import re
    return pytest.raises(RuntimeError, match="^" + re.escape(sentence) + "$")


def test_validator_sentences(hip):
    """The opening checks' sentences, word for word, on the smallest inputs that reach them."""
    from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec
    c = _codec(R.initial_params(0))
    with _raises_exactly("OnlineLanguageCodec: a GPU device is required (there is no torch fallback)"):
        OnlineLanguageCodec("cpu")
    with _raises_exactly("train_step: features must be a float32 tensor on the GPU"):
        c.train_step(torch.rand(2, 32), 1e-4)
    with _raises_exactly("encode: features must be a float32 tensor on the GPU"):
        c.encode(torch.rand(2, 32, device=DEV).double())
    with _raises_exactly("encode: features has shape (2, 31), expected [N,32] with N >= 1"):
        c.encode(torch.rand(2, 31, device=DEV))
    with _raises_exactly("decode: codes must be a float32 tensor on the GPU"):
        c.decode(torch.rand(2, 15, device=DEV).double())
    with _raises_exactly("decode: codes has shape (2, 31), expected [N,15] with N >= 1"):
        c.decode(torch.rand(2, 31, device=DEV))
