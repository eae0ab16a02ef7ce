"""Neither entry of include/olsr_clip_trunk.h writes outside the bytes of the outputs it names, nor outside the workspace it
asked for: the extents rows of olsr_convnext_block and olsr_clip_trunk_forward, the way tests/test_gpu_map_io_extents.py holds
its header's, on tests/extent_harness.py as it is.

| entry                   | sizes                                                   | why these                                       |
| olsr_convnext_block     | C = 64 and 320 on 5 x 7; C = 64 on 9 x 13               | 35 and 117 pixels: no multiple of the 64-pixel  |
|                         |                                                         | tile nor of the depthwise kernel's 4; 64: the   |
|                         |                                                         | fused block, 320: the three-launch block        |
|                         | C = 256 on 11 x 13                                      | the widest fused block, three tiles (143 pixels)|
| olsr_clip_trunk_forward | the small trunk (maps 8x8 ... 1x1, E = 48), image 20x27 | E = 48: the head's last neuron tile is partial  |
|                         | clip_trunk_ref's tiles64 (maps 16x16 ... 2x2, E = 16,   | four pixel tiles in the stem and stage 0; three |
|                         | R = 64), image 77x64                                    | waves of the head without neurons               |

Each entry runs three ways: plain buffers, guarded buffers (64 KiB of a known byte on either side; every output pre-filled
with a pattern no input holds), and guarded buffers whose inputs and outputs start 4 bytes past a 256-byte boundary.  The
workspace is guarded at exactly the bytes its _workspace_bytes asked for, 16-byte aligned as the contract has it.  Checked: the
guards are intact, every word of every output was stored, the inputs and the parameters are unchanged, and the guarded runs
give the plain run's bits."""
import ctypes as C

import pytest
import torch

import clip_trunk_ref as R
import extent_harness as H
from online_lang_splatting_amd import _abi

pytestmark = pytest.mark.gpu
DEV = H.DEV
F32 = torch.float32
COVERED = ("olsr_convnext_block", "olsr_clip_trunk_forward")
KW = dict(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512), embed_dim=48)


def _L():
    from online_lang_splatting_amd._lib import lib
    return lib()


def _check_rc(rc):
    from online_lang_splatting_amd._lib import check
    check(rc)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


@pytest.fixture(autouse=True)
def _forget_buffers():
    yield
    H.reset()


def _placed(t, misalign):
    if misalign is None:
        return t.to(DEV)
    g = H.guarded_tensor(t.shape, F32, misalign)
    g.copy_(t)
    return g


def _out(shape, misalign):
    return H.prefill(torch.empty(shape, dtype=F32, device=DEV)) if misalign is None else H.guarded_tensor(shape, F32, misalign)


@pytest.mark.parametrize("c,h,w", [(64, 5, 7), (320, 5, 7), (64, 9, 13), (256, 11, 13)])
def test_convnext_block(hip, c, h, w):
    from online_lang_splatting_amd import ClipTrunk
    L = _L()
    kw = dict(depths=(1, 1, 1, 1), dims=(c, 64, 64, 64), embed_dim=16)
    trunk = ClipTrunk(DEV, R.trunk_state(6, **kw), resolution=32, **kw)
    at = trunk._offset["visual.trunk.stages.0.blocks.0.conv_dw.weight"]
    n_block = 8 * c * c + 58 * c
    x = R.make_map(c, h, w, 6)
    nbytes = int(L.olsr_convnext_block_workspace_bytes(c, h, w))
    assert nbytes == (2 if c <= _abi.CLIP_TRUNK_FUSED_MAX_C else 6) * c * h * w * 4
    results = []
    for misalign in (None, 0, 4):
        H.reset()
        xin, y = _placed(x, misalign), _out((c, h, w), misalign)
        params = _placed(trunk.flat[at:at + n_block].cpu(), None if misalign is None else 0)
        work = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if misalign is None else H.guarded(nbytes, 0)
        p = _abi.OlsrConvnextBlockParams(C=c, h=h, w=w, ln_eps=R.EPS, workspace_bytes=nbytes)
        _check_rc(L.olsr_convnext_block(C.byref(p), xin.data_ptr(), params.data_ptr(), y.data_ptr(), work.data_ptr(), _stream()))
        if misalign is not None:
            assert y.data_ptr() % 256 == misalign and work.data_ptr() % 16 == 0
            H.check([y, xin, params, work], (), [y])
            assert H.same_bits(xin.cpu(), x) and H.same_bits(params.cpu(), trunk.flat[at:at + n_block].cpu())
        else:
            H.check([], (), [y])
        results.append(y.cpu())
    assert H.same_bits(results[0], trunk.block(x.to(DEV), 0, 0).cpu()), "the plain run differs from ClipTrunk.block"
    assert H.same_bits(results[1], results[0]) and H.same_bits(results[2], results[0]), "a guarded run differs from the plain run"


def test_clip_trunk_forward(hip):
    _forward_extents(KW, 32, (20, 27), 7, dict(res2=(64, 8, 8), res3=(128, 4, 4), clip_vis_dense=(48, 1, 1)))


def test_clip_trunk_forward_tiles64(hip):
    case = R.TRUNK_CASES["tiles64"]
    kw = {k: case[k] for k in ("depths", "dims", "embed_dim")}
    assert case["embed_dim"] == 16 and case["resolution"] == 64 and case["image"] == (77, 64)
    _forward_extents(kw, 64, case["image"], case["state_seed"], dict(res2=(64, 16, 16), res3=(128, 8, 8), clip_vis_dense=(16, 2, 2)))


def _forward_extents(kw, resolution, hw, seed, shapes):
    from online_lang_splatting_amd import ClipTrunk
    L = _L()
    trunk = ClipTrunk(DEV, R.trunk_state(seed, **kw), resolution=resolution, **kw)
    img = R.make_image(*hw, seed)
    nbytes = trunk.workspace().numel()
    flat = trunk.flat.cpu()
    results = []
    for misalign in (None, 0, 4):
        H.reset()
        x = _placed(img, misalign)
        outs = {k: _out(s, misalign) for k, s in shapes.items()}
        params = _placed(flat, None if misalign is None else 0)
        work = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if misalign is None else H.guarded(nbytes, 0)
        p = trunk._params(*hw, 0, nbytes)
        _check_rc(L.olsr_clip_trunk_forward(C.byref(p), x.data_ptr(), params.data_ptr(), outs["res2"].data_ptr(),
                                            outs["res3"].data_ptr(), outs["clip_vis_dense"].data_ptr(), work.data_ptr(), _stream()))
        if misalign is not None:
            H.check(list(outs.values()) + [x, params, work], (), list(outs.values()))
            assert H.same_bits(x.cpu(), img) and H.same_bits(params.cpu(), flat)
        else:
            H.check([], (), list(outs.values()))
        results.append({k: v.cpu() for k, v in outs.items()})
    own = trunk.forward(img.to(DEV))
    for k in shapes:
        assert H.same_bits(results[0][k], own[k].cpu()), f"{k}: the plain run differs from ClipTrunk.forward"
        for r in results[1:]:
            assert H.same_bits(r[k], results[0][k]), f"{k}: a guarded run differs from the plain run"
