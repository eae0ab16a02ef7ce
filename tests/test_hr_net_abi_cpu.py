"""The high-resolution net's C-ABI and host helpers without a GPU: the symbols load, _abi carries the sizes and the state list,
every argument error returns OLSR_ERR_ARG before anything touches the device, the workspace size is monotone, packing
round-trips, and the loader accepts what it should and names what it rejects."""
import ctypes as C

import pytest
import torch

import hr_net_ref as R
from online_lang_splatting_amd import _abi


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


SIZES = dict(h=24, w=24, h3=48, w3=48, h2=96, w2=96)


def _params(L, **kw):
    p = dict(SIZES, c_fv=768, c_f3=384, c_f2=192, c_out=768, launches=0, fv_stride=576, f3_stride=2304, f2_stride=9216,
             out_stride=36864, bn_eps=1e-5)
    p.update(kw)
    if "workspace_bytes" not in p:
        p["workspace_bytes"] = int(L.olsr_hr_net_workspace_bytes(24, 24, 48, 48, 96, 96))
    return _abi.OlsrHrNetParams(**p)


def test_symbols_and_abi(L):
    from online_lang_splatting_amd import _lib
    for s in ("olsr_hr_net_workspace_bytes", "olsr_hr_net_forward"):
        assert hasattr(L, s) and s in _lib.EXPORTS
    assert _abi.HR_NET_PARAMS == 19890816 == R.N_PACKED and _abi.HR_NET_LAUNCHES == 13 == len(_abi.HR_NET_LAYERS)
    assert tuple(_abi.HR_NET_CHANNELS) == (R.C_FV, R.C_F3, R.C_F2, R.C_OUT)
    assert tuple(_abi.HR_NET_LAYERS) == tuple(R.LAYERS) and tuple(_abi.HR_NET_STATE) == tuple(R.STATE)
    packed = sum(_abi.HR_NET_TAPS[kind] * o * i + o + (4 * o if bn else 0) for _, kind, o, i, bn in _abi.HR_NET_LAYERS)
    assert packed == _abi.HR_NET_PARAMS == sum(int(torch.Size(s).numel()) for _, s in _abi.HR_NET_STATE)
    # 10 int32, uint32 launches, 4 bytes of padding | 4 int64 strides | double bn_eps | uint64 workspace_bytes
    P = _abi.OlsrHrNetParams
    assert C.sizeof(P) == 96 and P.launches.offset == 40 and P.fv_stride.offset == 48 and P.out_stride.offset == 72
    assert P.bn_eps.offset == 80 and P.workspace_bytes.offset == 88
    import online_lang_splatting_amd as pkg
    assert pkg.HighResLanguageNet is not None and "HighResLanguageNet" in pkg.__all__


def test_workspace_bytes(L):
    f = L.olsr_hr_net_workspace_bytes
    base = f(24, 24, 48, 48, 96, 96)
    # X0 [512,h,w] | three [512,2h,2w] | three [256,4h,4w] | [128,8h,8w], float32
    assert base == 4 * 576 * (512 + 3 * 512 * 4 + 3 * 256 * 16 + 128 * 64)
    for k in range(6):
        for bad in (0, -1):
            args = [24, 24, 48, 48, 96, 96]
            args[k] = bad
            assert f(*args) == 0
        prev = 0
        for v in (1, 2, 3, 24, 25, 100):      # monotone in every size
            args = [24, 24, 48, 48, 96, 96]
            args[k] = v
            assert f(*args) >= prev and f(*args) > 0
            prev = f(*args)
    assert f(25, 24, 48, 48, 96, 96) > base and f(24, 25, 48, 48, 96, 96) > base


# Addresses that are never dereferenced: every row below must be rejected before a launch.
PTR = 0x1000


def test_argument_errors(L):
    need = int(L.olsr_hr_net_workspace_bytes(24, 24, 48, 48, 96, 96))
    bad_params = [(f"{k} = {v}", {k: v}) for k in SIZES for v in (0, -3)]
    bad_params += [("c_fv", dict(c_fv=512)), ("c_f3", dict(c_f3=192)), ("c_f2", dict(c_f2=384)), ("c_out", dict(c_out=32)),
                   ("c_fv = 0", dict(c_fv=0)), ("fv_stride", dict(fv_stride=575)), ("f3_stride", dict(f3_stride=2303)),
                   ("f2_stride", dict(f2_stride=9215)), ("out_stride", dict(out_stride=36863)), ("stride < 0", dict(fv_stride=-576)),
                   ("fv_stride beyond 2^31 / 768", dict(fv_stride=(1 << 31) // 768)), ("out_stride beyond", dict(out_stride=1 << 40)),
                   ("bn_eps = 0", dict(bn_eps=0.0)), ("bn_eps < 0", dict(bn_eps=-1e-5)), ("bn_eps NaN", dict(bn_eps=float("nan"))),
                   ("workspace one byte short", dict(workspace_bytes=need - 1)), ("workspace 0", dict(workspace_bytes=0)),
                   ("workspace of a smaller map", dict(workspace_bytes=int(L.olsr_hr_net_workspace_bytes(23, 24, 48, 48, 96, 96)))),
                   ("launch 13", dict(launches=1 << 13))]
    # params, fv, f3, f2, packed_params, workspace, out, stream
    ok = [_params(L), PTR, PTR, PTR, PTR, PTR, PTR, None]
    rows = [("params struct", {0: None})] + [(f"argument {k} NULL", {k: None}) for k in range(1, 7)]
    rows += [("packed_params alignment", {4: PTR + 4}), ("workspace alignment", {5: PTR + 8})]
    rows += [(what, {0: _params(L, **kw)}) for what, kw in bad_params]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        a0 = None if args[0] is None else C.byref(args[0])
        assert L.olsr_hr_net_forward(a0, *args[1:]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(b"hr_net_forward"), what
    assert L.olsr_hr_net_forward(C.byref(_params(L, c_f3=192)), *ok[1:]) == _abi.OLSR_ERR_ARG
    assert b"fv 768, f3 384, f2 192, out 768" in L.olsr_last_error()


def test_packing_round_trips_and_names_what_it_rejects():
    from online_lang_splatting_amd import hr_net
    state = R.net_state(300)
    flat = torch.zeros(_abi.HR_NET_PARAMS)
    hr_net.load_hr_state(flat, state)
    back = hr_net.unpack_hr_state(flat)
    assert list(back) == [k for k, _ in R.STATE]
    for k, v in state.items():
        assert torch.equal(back[k], v) and back[k].is_contiguous(), k
    # a tap's [out][in] slab is contiguous: Conv2d [o,i,ky,kx] -> slab 3 ky + kx, ConvTranspose2d [i,o,ky,kx] -> slab 4 ky + kx
    views = hr_net.packed_views(flat)
    w = state["initial_conv.0.weight"]
    assert tuple(views["initial_conv.0.weight"].shape) == (9, 512, 768)
    assert torch.equal(views["initial_conv.0.weight"][3 * 2 + 1], w[:, :, 2, 1])
    assert views["initial_conv.0.weight"].data_ptr() == flat.data_ptr()
    wt = state["upsample2.0.weight"]
    assert tuple(views["upsample2.0.weight"].shape) == (16, 256, 512)
    assert torch.equal(views["upsample2.0.weight"][4 * 3 + 2], wt[:, :, 3, 2].t())
    assert torch.equal(views["final_conv.bias"], state["final_conv.bias"])
    assert views["final_conv.bias"].data_ptr() == flat.data_ptr() + 4 * (_abi.HR_NET_PARAMS - 768)
    assert all((v.data_ptr() - flat.data_ptr()) % 16 == 0 for k, v in views.items() if k.endswith(".weight") or k.endswith(".bias"))
    # a Lightning checkpoint of LangSupervisedNet, its state_dict, num_batches_tracked
    full = dict(state, **{f"{bn}.num_batches_tracked": torch.tensor(7) for bn in R.BN_PATHS})
    for s in (full, {"model." + k: v for k, v in full.items()}, {"epoch": 3, "state_dict": {"model." + k: v for k, v in full.items()}}):
        again = torch.zeros_like(flat)
        hr_net.load_hr_state(again, s)
        assert torch.equal(again, flat)
    with pytest.raises(RuntimeError, match=r"missing keys \['upsample1.1.running_var'\]"):
        hr_net.load_hr_state(flat, {k: v for k, v in state.items() if k != "upsample1.1.running_var"})
    with pytest.raises(RuntimeError, match=r"unexpected keys \['final_conv.2.weight'\]"):
        hr_net.load_hr_state(flat, dict(state, **{"final_conv.2.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"attention_fusion2.fusion.0.weight has shape \(256, 256, 3, 3\)"):
        hr_net.load_hr_state(flat, dict(state, **{"attention_fusion2.fusion.0.weight": torch.zeros(256, 256, 3, 3)}))
    with pytest.raises(RuntimeError, match=r"upsample1.0.weight has shape \(512, 512, 3, 3\)"):
        hr_net.load_hr_state(flat, dict(state, **{"upsample1.0.weight": torch.zeros(512, 512, 3, 3)}))
    with pytest.raises(RuntimeError, match="checkpoint or state dict"):
        hr_net.load_hr_state(flat, [1, 2])
    with pytest.raises(RuntimeError, match="packed array"):
        hr_net.packed_views(torch.zeros(_abi.HR_NET_PARAMS - 1))


def test_no_cpu_fallback():
    from online_lang_splatting_amd import hr_net
    with pytest.raises(RuntimeError, match="GPU device is required"):
        hr_net.HighResLanguageNet("cpu")
