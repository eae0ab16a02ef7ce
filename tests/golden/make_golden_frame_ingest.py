"""Generates tests/golden/frame_ingest.npz by executing the REFERENCE's own statements on the CPU.  Runs ONLY where the
reference checkout exists (OLSR_REFERENCE names it); the committed .npz is data (arrays only).

MonocularDataset.__getitem__ (utils/dataset.py:316-350; ReplicaDataset and TUMDataset inherit it) reads its files with PIL; its two statements that this project restates —
the assignment of `depth` (np.array(Image.open(depth_path)) / self.depth_scale) and the final assignment of `image`
(torch.from_numpy(image / 255.0).clamp(0.0, 1.0).permute(2, 0, 1).to(...)) — are taken out of the method by `ast` and executed
as they stand on synthetic arrays: `Image.open` hands back the array, `self` is a stub with depth_scale, device "cpu" and
dtype float32.  The depth is then narrowed as the reference's consumers narrow it (get_loss_tracking / add_new_keyframe:
torch.from_numpy(depth).to(dtype=torch.float32))."""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if "OLSR_REFERENCE" not in os.environ:
    raise SystemExit("set OLSR_REFERENCE to the reference checkout")
REF = os.environ["OLSR_REFERENCE"]
sys.path.insert(0, os.path.dirname(HERE))
import frame_ingest_ref as R  # noqa: E402


def reference_statements():
    tree = ast.parse(open(os.path.join(REF, "utils", "dataset.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MonocularDataset")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__getitem__")
    found = {}
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            name, src = node.targets[0].id, ast.unparse(node)
            if name == "depth" and "depth_scale" in src:
                found["depth"] = node
            if name == "image" and "255.0" in src:
                found["image"] = node
    assert set(found) == {"depth", "image"}
    return {k: compile(ast.Module(body=[v], type_ignores=[]), f"<reference {k}>", "exec") for k, v in found.items()}


def run_reference(code, rgb, depth, depth_scale):
    ns = dict(np=np, torch=torch, Image=types.SimpleNamespace(open=lambda a: a), depth_path=depth, image=rgb,
              self=types.SimpleNamespace(depth_scale=depth_scale, device="cpu", dtype=torch.float32))
    exec(code["depth"], ns)
    exec(code["image"], ns)
    d = torch.from_numpy(np.asarray(ns["depth"])).to(dtype=torch.float32)
    return ns["image"].contiguous().numpy(), d.numpy()


CASES = [("all256_u16", 64, 4, np.uint16, 6553.5), ("odd_u16", 67, 5, np.uint16, 5000.0),
         ("odd_f32", 67, 5, np.float32, 6553.5), ("all256_f32", 64, 4, np.float32, 5000.0)]

if __name__ == "__main__":
    code = reference_statements()
    out = {"names": np.array([c[0] for c in CASES])}
    for k, (name, W, H, dt, scale) in enumerate(CASES):
        rgb, depth = R.synthetic_frame(W, H, dt, seed=100 + k)
        image, d = run_reference(code, rgb, depth, scale)
        assert image.dtype == np.float32 and image.shape == (3, H, W) and d.dtype == np.float32 and d.shape == (H, W)
        out.update({f"{name}_rgb": rgb, f"{name}_depth_in": depth, f"{name}_scale": np.float64(scale), f"{name}_image": image,
                    f"{name}_depth": d})
    np.savez_compressed(os.path.join(HERE, "frame_ingest.npz"), **out)
    print("wrote frame_ingest.npz:", ", ".join(c[0] for c in CASES))
