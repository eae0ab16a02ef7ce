"""Mapping's bundle adjustment without a GPU: the symbols load, the structs and constants mirror include/olsr.h, every
argument error returns OLSR_ERR_ARG before any launch (the pointers below are never dereferenced), and the host layer refuses
CPU tensors."""
import ctypes as C
import os

import pytest
import torch

from online_lang_splatting_amd import _abi

PTR = 0x1000
ENTRIES = ("olsr_window_pose_step", "olsr_isotropic_reg_scratch_bytes", "olsr_isotropic_reg", "olsr_adam_step_groups_reg")


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


def test_symbols_structs_and_exports(L):
    from online_lang_splatting_amd import _lib
    for s in ENTRIES:
        assert hasattr(L, s) and s in _lib.EXPORTS
    R = _abi.OlsrAdamReg
    assert C.sizeof(R) == 16 and (R.isotropic_weight.offset, R.activations.offset, R.P_total.offset) == (0, 8, 12)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "olsr.h")).read()
    for line in ("#define OLSR_WINDOW_MAX_VIEWS 32", "#define OLSR_WINDOW_OPT_POSE 1", "#define OLSR_WINDOW_OPT_EXPOSURE 2",
                 "typedef struct olsr_adam_reg {", "double isotropic_weight;", "int32_t activations;", "int32_t P_total;"):
        assert line in header, line
    assert (_abi.WINDOW_MAX_VIEWS, _abi.WINDOW_OPT_POSE, _abi.WINDOW_OPT_EXPOSURE) == (32, 1, 2)
    assert L.olsr_isotropic_reg_scratch_bytes(1) >= 8
    assert L.olsr_isotropic_reg_scratch_bytes(500_000) >= 8 * ((500_000 + 255) // 256)
    import online_lang_splatting_amd as pkg
    for name in ("KeyframeWindow", "isotropic_loss"):
        assert getattr(pkg, name) is not None and name in pkg.__all__


def _pose_params():
    return _abi.OlsrPoseParams(lr_rot=0.0015, lr_trans=0.0005, lr_exposure=0.01, beta1=0.9, beta2=0.999, eps=1e-8,
                               converged_threshold=1e-4, step=1)


def _flags(*f):
    return (C.c_int32 * len(f))(*f)


def test_window_pose_step_argument_errors(L):
    def call(V=3, flags=_flags(0, 3, 2), params=True, tau=PTR, exposure=PTR, proj=PTR, state=PTR, status=PTR):
        return L.olsr_window_pose_step(C.byref(_pose_params()) if params else None, V, flags, tau, exposure, proj, state, status,
                                       None, None)
    rows = dict(V0=dict(V=0), Vneg=dict(V=-1), V33=dict(V=33, flags=_flags(*([0] * 33))), unknown_bits=dict(flags=_flags(0, 4, 2)),
                negative_flag=dict(flags=_flags(0, -1, 2)), params=dict(params=False), flags=dict(flags=None), proj=dict(proj=None),
                state=dict(state=None), status=dict(status=None), tau_needed=dict(tau=None), exposure_needed=dict(exposure=None),
                tau_needed_pose_only=dict(flags=_flags(0, 1, 0), tau=None, exposure=None),
                exposure_needed_alone=dict(flags=_flags(0, 0, 2), tau=None, exposure=None))
    for what, kw in rows.items():
        assert call(**kw) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"window_pose_step: "), (what, L.olsr_last_error())


def test_isotropic_reg_argument_errors(L):
    def call(P=100, scales=PTR, act=_abi.ACT_SCALE_EXP, weight=10.0, grad=PTR, loss=PTR, scratch=PTR):
        return L.olsr_isotropic_reg(P, scales, act, weight, grad, loss, scratch, None)
    rows = dict(Pneg=dict(P=-1), scales=dict(scales=None), activations=dict(act=8), activations_neg=dict(act=-1),
                weight_nan=dict(weight=float("nan")), weight_inf=dict(weight=float("inf")), loss_without_scratch=dict(scratch=None))
    for what, kw in rows.items():
        assert call(**kw) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"isotropic_reg: "), (what, L.olsr_last_error())
    assert call(grad=None, loss=None, scratch=None) == _abi.OLSR_OK   # nothing asked for: nothing launched


def test_adam_step_groups_reg_argument_errors(L):
    P, M, F = 100, 1, 0
    gp = _abi.OlsrAdamGroupParams(base=_abi.OlsrAdamParams(beta1=0.9, beta2=0.999, eps=1e-15, step=1), skip_mask=0)
    for g in range(7):
        gp.group_step[g] = 1
    flats = (C.c_void_p * 1)(PTR)

    def call(reg, params=gp, P=P, scales=PTR):
        return L.olsr_adam_step_groups_reg(P, M, F, C.byref(params) if params is not None else None, 1, flats, None, PTR, PTR, PTR,
                                           scales, PTR, None, PTR, PTR, C.byref(reg) if reg is not None else None, None)
    reg = lambda **kw: _abi.OlsrAdamReg(**dict(dict(isotropic_weight=10.0, activations=_abi.ACT_ALL, P_total=P), **kw))  # noqa: E731
    for what, r in (("P_total < P", reg(P_total=P - 1)), ("P_total = 0", reg(P_total=0)), ("activations", reg(activations=8)),
                    ("weight nan", reg(isotropic_weight=float("nan")))):
        assert call(r) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"adam_step_groups_reg: "), (what, L.olsr_last_error())
    # the checks of olsr_adam_step_groups hold with and without a regulariser
    for r in (None, reg(), reg(isotropic_weight=0.0, P_total=0)):
        assert call(r, params=None) == _abi.OLSR_ERR_ARG
        assert call(r, scales=None) == _abi.OLSR_ERR_ARG
        assert call(r, P=-1) == _abi.OLSR_ERR_ARG
        assert call(r, P=0) == _abi.OLSR_OK


def test_host_layer_needs_a_gpu():
    from online_lang_splatting_amd import KeyframeWindow, isotropic_loss
    with pytest.raises(RuntimeError, match="GPU"):
        KeyframeWindow(torch.eye(4).repeat(2, 1, 1), [0, 1], torch.eye(4), 1.0, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        isotropic_loss(torch.ones(5, 3))
