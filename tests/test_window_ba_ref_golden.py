"""tests/window_ba_ref.py against tests/golden/window_ba.npz — the reference's own keyframe_optimizers.step() + update_pose
over a five-view window, and its isotropic regulariser under autograd — on the CPU.  Tolerances are those of
tests/test_gpu_pose.py for the poses (torch's CPU Adam fuses multiply-adds, the Camera inverts [R|t] twice); for the
regulariser 6 * 2^-24 relative to the float64 statement on rows with a gradient, exactly zero on rows of three equal scales."""
import os

import numpy as np

import window_ba_ref as ref

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_ba.npz"))


def golden_flags():
    pw = int(G["pose_window"])
    return [0 if uid == 0 else (ref.POSE | ref.EXPOSURE if v < pw else ref.EXPOSURE) for v, uid in enumerate(G["uids"])]


def test_window_step_follows_the_references_window_optimiser():
    flags = golden_flags()
    assert flags == [0, 3, 3, 2, 2]
    st = ref.make_states(G["R0"], G["T0"], G["exposure0"])
    status = np.zeros((len(flags), 2), dtype=np.int32)
    lrs = tuple(float(x) for x in G["lr"])
    start = st.copy()
    for i in range(len(G["grad_tau"])):
        ref.window_step(st, status, flags, G["grad_tau"][i], G["grad_exposure"][i], G["proj"], lrs, step=i + 1)
        tol = 5e-7 * (i + 1)
        for v, fl in enumerate(flags):
            T = st[v, :16].reshape(4, 4)
            np.testing.assert_allclose(T[:3, :3], G["R"][i, v], rtol=0, atol=tol)
            np.testing.assert_allclose(T[:3, 3], G["T"][i, v], rtol=0, atol=tol)
            np.testing.assert_allclose(st[v, 16:32].reshape(4, 4), G["view"][i, v], rtol=0, atol=tol)
            scale = np.abs(G["full"][i, v]).max()
            np.testing.assert_allclose(st[v, 32:48].reshape(4, 4), G["full"][i, v], rtol=0, atol=1e-6 * scale * (i + 1))
            np.testing.assert_allclose(st[v, 48:51], G["campos"][i, v], rtol=0, atol=1e-6 * (i + 1))
            np.testing.assert_allclose(st[v, 70:72], G["exposure"][i, v], rtol=2e-6, atol=1e-9)
            if fl & ref.POSE:
                np.testing.assert_allclose(st[v, 64:70], G["tau"][i, v], rtol=2e-6, atol=2e-6 * max(lrs[:2]))
            else:   # no pose group: pose and its optimiser words keep their bits
                assert st[v, :16].tobytes() == start[v, :16].tobytes() and not st[v, 52:70].any()
            assert status[v, 1] == (i + 1 if fl else 0)
    assert st[0, 70:76].tobytes() == start[0, 70:76].tobytes()   # frame 0: nothing at all


def test_regulariser_restatement_against_autograd():
    x, weight = G["reg_x"], float(G["reg_weight"])
    for P in G["reg_sizes"]:
        P = int(P)
        c = weight / (3.0 * P)
        equal = np.arange(P) % 3 == 0   # rows of three equal scales: exactly zero, whatever the float32 mean is (the goldens
        real = ~equal                   # hold autograd's rounding residue there at some P)
        # activated: the statement on scaling itself
        s = G["reg_s"][:P]
        r, _ = ref.isotropic_rows(s, False, weight)
        g64 = G[f"reg_act_grad64_P{P}"]
        assert not r[equal].any() and (np.abs(r - g64)[real] <= 6 * 2.0 ** -24 * np.abs(g64)[real]).all(), P
        assert abs(ref.isotropic_loss(s, False, weight) - float(G[f"reg_act_loss64_P{P}"])) <= 6 * 2.0 ** -24 * weight * s.max()
        # raw: through exp
        r, _ = ref.isotropic_rows(x[:P], True, weight)
        g64 = G[f"reg_grad64_P{P}"]
        assert not r[equal].any() and (np.abs(r - g64)[real] <= 6 * 2.0 ** -24 * np.abs(g64)[real]).all(), P
        assert abs(ref.isotropic_loss(x[:P], True, weight) - float(G[f"reg_loss64_P{P}"])) <= 6 * 2.0 ** -24 * weight * s.max()
        # float32 autograd: the same to a few ulp of c (its own rounding of c sg - mean(c sg))
        np.testing.assert_allclose(r, G[f"reg_grad32_P{P}"], rtol=0, atol=8 * 2.0 ** -24 * c * s.max())


def test_p_total_scales_the_gradient_only():
    x, weight = G["reg_x"][:65], float(G["reg_weight"])
    r, _ = ref.isotropic_rows(x, True, weight, P_total=4099)
    full, _ = ref.isotropic_rows(G["reg_x"], True, weight)
    assert r.tobytes() == full[:65].tobytes()
