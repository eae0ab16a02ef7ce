"""The numpy restatement of a frame's ingest (tests/frame_ingest_ref.py) against what the reference's own statements compute
on the CPU (tests/golden/frame_ingest.npz, recorded by tests/golden/make_golden_frame_ingest.py): equal bit for bit."""
import os

import numpy as np
import pytest

import frame_ingest_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_ingest.npz"))
NAMES = [str(n) for n in GOLD["names"]]


def test_golden_covers_the_cases_the_contract_names():
    shapes = {tuple(GOLD[f"{n}_rgb"].shape[:2]) for n in NAMES}
    assert {(4, 64), (5, 67)} <= shapes                      # 64 x 4 and 67 x 5 pixels
    assert {float(GOLD[f"{n}_scale"]) for n in NAMES} == {6553.5, 5000.0}
    assert {GOLD[f"{n}_depth_in"].dtype for n in NAMES} == {np.dtype(np.uint16), np.dtype(np.float32)}
    for n in NAMES:
        rgb = GOLD[f"{n}_rgb"]
        for c in range(3):
            assert len(np.unique(rgb[..., c])) == 256, (n, c)
    u16 = np.concatenate([GOLD[f"{n}_depth_in"].ravel() for n in NAMES if GOLD[f"{n}_depth_in"].dtype == np.uint16])
    assert {0, 1, 65535} <= set(u16.tolist())


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    image, depth = R.ingest(GOLD[f"{name}_rgb"], GOLD[f"{name}_depth_in"], float(GOLD[f"{name}_scale"]))
    gi, gd = GOLD[f"{name}_image"], GOLD[f"{name}_depth"]
    assert image.dtype == gi.dtype == np.float32 and image.shape == gi.shape
    assert depth.dtype == gd.dtype == np.float32 and depth.shape == gd.shape
    assert image.tobytes() == gi.tobytes()
    assert depth.tobytes() == gd.tobytes()
    assert image.min() == 0.0 and image.max() == 1.0
