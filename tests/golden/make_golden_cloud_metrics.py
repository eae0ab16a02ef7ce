"""Generates tests/golden/cloud_metrics.npz: what the reference's 3-D evaluation computes on the seeded clouds of
tests/cloud_metrics_ref.cases().  Runs ONLY where the reference checkout exists (OLSR_REFERENCE names it); the committed .npz is
data (arrays only).

Chamfer is recorded from the reference's OWN chamfer_distance
(tsdf-fusion/3d_evaluation_and_visualize_langslam_dim15.py:235-274) with scikit-learn's kd-tree (1.7 where this file was made).
That script runs a whole evaluation when it is imported, so only that one function is executed: its definition is taken out of
the parsed source by name and compiled on its own, with sklearn's NearestNeighbors in its globals.

The EMD is NOT recorded from the reference: its kernel (tsdf-fusion/PyTorchEMD/cuda/emd_kernel.cu) is CUDA only and cannot run
where this file is made.  `emd_cost` / `emd_residual` are tests/cloud_metrics_ref.emd_ref in float64 — a RESTATEMENT of the
algorithm, recorded so that the tests notice when the restatement itself changes, not evidence about the reference.  The one
piece of evidence about the reference is the hand case of its PyTorchEMD/test_emd_loss.py (two points against two, a batch of
three), whose hand-computed answer is 0.71 / 2 = 0.355 per item; its points are stored as hand_p1 / hand_p2.

Per case: names, n, m, checksum (the float64 sum of all coordinates: the tests regenerate the clouds from the seed and compare),
chamfer [cases,3] (x_to_y, y_to_x, bi), emd_cost, emd_residual [cases,2]."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if "OLSR_REFERENCE" not in os.environ:
    raise SystemExit("set OLSR_REFERENCE to the reference checkout")
sys.path.insert(0, os.path.dirname(HERE))
import cloud_metrics_ref as R  # noqa: E402

SCRIPT = os.path.join(os.environ["OLSR_REFERENCE"], "tsdf-fusion", "3d_evaluation_and_visualize_langslam_dim15.py")


def reference_chamfer():
    from sklearn.neighbors import NearestNeighbors
    tree = ast.parse(open(SCRIPT).read(), SCRIPT)
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "chamfer_distance"]
    assert len(fn) == 1
    scope = {"np": np, "NearestNeighbors": NearestNeighbors}
    exec(compile(ast.Module(body=fn, type_ignores=[]), SCRIPT, "exec"), scope)
    return scope["chamfer_distance"]


def main():
    import sklearn
    chamfer = reference_chamfer()
    cases = R.cases()
    names = sorted(cases)
    out = dict(names=np.array(names), n=[], m=[], checksum=[], chamfer=[], emd_cost=[], emd_residual=[])
    for name in names:
        x, y = cases[name]
        out["n"].append(x.shape[0])
        out["m"].append(y.shape[0])
        out["checksum"].append(float(x.astype(np.float64).sum() + y.astype(np.float64).sum()))
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        out["chamfer"].append([float(chamfer(x64, y64, direction=d)) for d in ("x_to_y", "y_to_x", "bi")])
        mine = R.chamfer_ref(x, y)
        e = R.emd_ref(x, y)
        out["emd_cost"].append(e["cost"])
        out["emd_residual"].append(e["residual"])
        print(f"{name:>18}: chamfer bi {out['chamfer'][-1][2]:.9g} (brute force differs by {abs(mine['bi'] - out['chamfer'][-1][2]):.2e}), "
              f"emd {e['emd']:.9g}, residual {e['residual'][0]:.3e} {e['residual'][1]:.3e}")
    out = {k: np.asarray(v) for k, v in out.items()}
    out["hand_p1"], out["hand_p2"], out["hand_emd"] = R.HAND_P1, R.HAND_P2, np.float64(R.HAND_EMD)
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(os.path.join(HERE, "cloud_metrics.npz"), **out)


if __name__ == "__main__":
    main()
