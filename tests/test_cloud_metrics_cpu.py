"""Point-cloud metrics, the part that needs no GPU: the numpy yardsticks against the hand case and the fixture recorded from
the reference, the library's symbols, the entries' argument checks (they return before any launch) and the Python functions'
refusals (there is no torch fallback)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cloud_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000   # a made-up address: every call below returns before anything could follow it


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import build
    build.build()
    from online_lang_splatting_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "cloud_metrics.npz"))


def test_emd_ref_reproduces_the_hand_case(golden):
    assert np.array_equal(golden["hand_p1"], R.HAND_P1) and np.array_equal(golden["hand_p2"], R.HAND_P2)
    got = R.emd_ref(R.HAND_P1, R.HAND_P2)
    assert abs(got["emd"] - float(golden["hand_emd"])) <= 1e-6 and float(golden["hand_emd"]) == 0.355, got
    for order, exp in R.VARIANTS:
        assert abs(R.emd_ref(R.HAND_P1, R.HAND_P2, np.float32, order, exp)["emd"] - 0.355) <= 1e-6


def test_cost_per_level_equals_the_dense_match_matrix():
    # adding d * w level by level is the reference's sum d * match over the matrix the levels' w accumulate into
    cases = R.cases()
    for name in ("hand_2_2", "uniform_5_3", "uniform_3_5", "uniform_65_63", "uniform_255_257", "reversed_257"):
        got = R.emd_ref(*cases[name], dense=True)
        assert abs(got["cost"] - got["cost_dense"]) <= 64 * 2.0 ** -53 * abs(got["cost_dense"]), (name, got)


def test_multipliers_are_integer_quotients():
    # 5 against 3: both multipliers are 1, so two units of the left mass stay unassigned
    x, y = R.cases()["uniform_5_3"]
    assert abs(R.emd_ref(x, y)["residual"][0] - 2.0) < 1e-6
    assert abs(R.emd_ref(y, x)["residual"][1] - 2.0) < 1e-6


def test_fixture_matches_the_seeded_cases_and_the_yardsticks(golden):
    cases = R.cases()
    assert sorted(cases) == [str(s) for s in golden["names"]]
    for i, name in enumerate(golden["names"]):
        x, y = cases[str(name)]
        assert (x.shape[0], y.shape[0]) == (int(golden["n"][i]), int(golden["m"][i]))
        assert float(x.astype(np.float64).sum() + y.astype(np.float64).sum()) == float(golden["checksum"][i]), name
        # the reference's own chamfer_distance (kd-tree, float64) against brute force in float64
        mine = R.chamfer_ref(x, y)
        want = golden["chamfer"][i]
        got = np.array([mine["x_to_y"], mine["y_to_x"], mine["bi"]])
        assert np.all(np.abs(got - want) <= 8 * 2.0 ** -53 * np.abs(want)), (name, got, want)
        if x.shape[0] * y.shape[0] <= 70000:   # (the restatement's record, where it is cheap)
            e = R.emd_ref(x, y)
            assert abs(e["cost"] - float(golden["emd_cost"][i])) <= 1e-12 * abs(e["cost"]), name


def test_chamfer_ref_takes_the_first_index_on_ties():
    x = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    y = np.array([[2, 0, 0], [0.5, 0, 0], [0.5, 0, 0]], np.float32)
    got = R.chamfer_ref(x, y, np.float32)
    assert got["nn_x"].tolist() == [1, 1] and got["nn_y"].tolist() == [1, 0, 0]
    assert got["min_d2_x"].tolist() == [0.25, 0.25] and got["min_d2_y"].tolist() == [1.0, 0.25, 0.25]
    assert got["x_to_y"] == 0.5 and abs(got["y_to_x"] - 2.0 / 3.0) < 1e-15 and got["bi"] == got["y_to_x"] + got["x_to_y"]


def test_library_exports_the_entries(L):
    from online_lang_splatting_amd import _abi, _lib
    names = ("olsr_emd_scratch_bytes", "olsr_emd_cost", "olsr_chamfer_scratch_bytes", "olsr_chamfer")
    src = open(os.path.join(ROOT, "include", "olsr.h")).read()
    for s in names:
        assert s in _lib.EXPORTS and hasattr(L, s) and s + "(" in src
    assert f"#define OLSR_CLOUD_MAX_SEGMENTS {_abi.CLOUD_MAX_SEGMENTS}\n" in src
    # O(n + m): doubling both clouds at most doubles the scratch (plus alignment), and B only adds the parked offsets
    one, two = L.olsr_emd_scratch_bytes(1, 10000, 10000), L.olsr_emd_scratch_bytes(1, 20000, 20000)
    assert 10000 * (8 + 12 + 48 * 4 + 8 + 16 * 4) <= one <= two <= 2 * one
    assert L.olsr_emd_scratch_bytes(7, 10000, 10000) - one <= 2 * 256 + 64
    assert 20000 * 16 * 8 <= L.olsr_chamfer_scratch_bytes(1, 10000, 10000) <= 20000 * 16 * 8 + 4096
    assert L.olsr_emd_scratch_bytes(0, -5, -5) <= 4096


def test_entries_validate_their_arguments(L):
    from online_lang_splatting_amd import _abi
    ARG = _abi.OLSR_ERR_ARG
    i32 = C.c_int32

    def table(*v):
        return (i32 * len(v))(*v)
    ok1, ok2 = table(0, 5, 5, 9), table(0, 3, 7, 7)

    def emd(B=3, off1=ok1, off2=ok2, max1=5, max2=4, xyz1=X, xyz2=X, cost=X, residual=X, valid=X, scratch=X):
        return L.olsr_emd_cost(B, off1, off2, max1, max2, xyz1, xyz2, cost, residual, valid, scratch, None)

    def chamfer(B=3, off1=ok1, off2=ok2, max1=5, max2=4, xyz1=X, xyz2=X, d1=X, n1=X, d2=X, n2=X, mean=X, valid=X, scratch=X):
        return L.olsr_chamfer(B, off1, off2, max1, max2, xyz1, xyz2, d1, n1, d2, n2, mean, valid, scratch, None)
    rows = [
        ("emd B = 0", lambda: emd(B=0), "emd_cost: B must be between 1 and 32767"),
        ("emd B < 0", lambda: emd(B=-1), "emd_cost: B must be between 1 and 32767"),
        ("emd B large", lambda: emd(B=32768), "emd_cost: B must be between 1 and 32767"),
        ("emd no offsets", lambda: emd(off2=None), "emd_cost: off1 and off2 are required"),
        ("emd max_n", lambda: emd(max1=-1), "emd_cost: max_n1 and max_n2 must be >= 0"),
        ("emd no cost", lambda: emd(cost=None), "emd_cost: every output is required"),
        ("emd no valid", lambda: emd(valid=None), "emd_cost: every output is required"),
        ("emd no scratch", lambda: emd(scratch=None), "emd_cost: scratch is required"),
        ("emd decreasing", lambda: emd(off1=table(0, 5, 4, 9)), "emd_cost: off1 must be non-decreasing"),
        ("emd decreasing 2", lambda: emd(off2=table(0, 3, 7, 6)), "emd_cost: off2 must be non-decreasing"),
        ("emd negative", lambda: emd(off1=table(-1, 4, 4, 4)), "emd_cost: off1[0] must be >= 0"),
        ("emd total", lambda: emd(B=1, off1=table(0, 2 ** 31 // 3), max1=2 ** 31 - 1), "emd_cost: off1[B] must be below 2^31 / 3"),
        ("emd longer", lambda: emd(max2=3), "emd_cost: a segment of off2 is longer than its max_n"),
        ("chamfer B", lambda: chamfer(B=0), "chamfer: B must be between 1 and 32767"),
        ("chamfer no offsets", lambda: chamfer(off1=None), "chamfer: off1 and off2 are required"),
        ("chamfer no mean", lambda: chamfer(mean=None), "chamfer: every output is required"),
        ("chamfer no valid", lambda: chamfer(valid=None), "chamfer: every output is required"),
        ("chamfer no min_d2_1", lambda: chamfer(d1=None), "chamfer: every output is required"),
        ("chamfer no nn_1", lambda: chamfer(n1=None), "chamfer: every output is required"),
        ("chamfer no min_d2_2", lambda: chamfer(d2=None), "chamfer: every output is required"),
        ("chamfer no nn_2", lambda: chamfer(n2=None), "chamfer: every output is required"),
        ("chamfer no xyz", lambda: chamfer(xyz2=None), "chamfer: xyz1 and xyz2 are required"),
        ("emd no xyz", lambda: emd(xyz1=None), "emd_cost: xyz1 and xyz2 are required"),
        ("chamfer no scratch", lambda: chamfer(scratch=None), "chamfer: scratch is required"),
        ("chamfer decreasing", lambda: chamfer(off2=table(0, 3, 2, 7)), "chamfer: off2 must be non-decreasing"),
        ("chamfer longer", lambda: chamfer(max1=4), "chamfer: a segment of off1 is longer than its max_n"),
    ]
    wrong = []
    for label, call, message in rows:
        rc = call()
        got = L.olsr_last_error().decode()
        if rc != ARG or got != message:
            wrong.append((label, rc, got))
    assert not wrong, wrong


def test_python_side_without_a_gpu():
    import online_lang_splatting_amd as pkg
    from online_lang_splatting_amd import cloud_metrics as M
    for name in ("earth_mover_distance", "emd_segments", "chamfer_distance", "chamfer_segments", "evaluate_classes"):
        assert getattr(pkg, name) is getattr(M, name) and name in pkg.__all__
    p = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match="xyz1 and xyz2 must be tensors on the GPU"):
        M.earth_mover_distance(p, p, transpose=False)
    with pytest.raises(RuntimeError, match="xyz2 must be float32"):
        M.earth_mover_distance(p, p.double(), transpose=False)
    with pytest.raises(RuntimeError, match=r"must be \(b, n, 3\) after the transpose"):
        M.earth_mover_distance(p, p)
    with pytest.raises(RuntimeError, match=r"xyz1 has shape \(4,\)"):
        M.earth_mover_distance(p[:, 0], p)
    with pytest.raises(RuntimeError, match="xyz1 has a batch of 2, xyz2 of 3"):
        M.earth_mover_distance(torch.zeros((2, 4, 3)), torch.zeros((3, 5, 3)), transpose=False)
    with pytest.raises(RuntimeError, match="xyz1 must be float32"):
        M.emd_segments(p.half(), [0, 4], p, [0, 4])
    with pytest.raises(RuntimeError, match=r"x has shape \(3, 4\), expected \[N,3\]"):
        M.chamfer_distance(p.t(), p)
    with pytest.raises(RuntimeError, match="x must be a tensor on the GPU"):
        M.chamfer_segments(p.numpy(), [0, 4], p, [0, 4])
    with pytest.raises(RuntimeError, match="xyz1 must be a tensor on the GPU"):
        M.emd_segments(p, [0, 4], p, [0, 4])
    with pytest.raises(RuntimeError, match="x must be a tensor on the GPU"):
        M.chamfer_distance(p, p)
    with pytest.raises(RuntimeError, match="points must be a tensor on the GPU"):
        M.evaluate_classes(p, torch.zeros(4, dtype=torch.int64), p, torch.zeros(4, dtype=torch.int64), [(0, 0)])
    with pytest.raises(RuntimeError, match="direction must be"):
        M.chamfer_distance(p, p, direction="both")
