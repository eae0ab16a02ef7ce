"""Records tests/golden/bwd_visit.npz: the backward's gradients on the scenes of tests/bwd_visit_scenes.py, as the build of the
commit BEFORE render_bwd_kernel staged one LDS record per entry and formed its row address on the scalar unit computes them.
tests/test_gpu_bwd_visit.py holds every later build to the same bits.

Run on a GPU, with that build selected:
    OLSR_LIB=/path/to/libolsr_of_that_commit.so OLSR_BINDING=ctypes python tests/golden/make_golden_bwd_visit.py

The fixture holds one SHA-256 per case over the fp32 bits of every gradient tensor (bwd_visit_scenes.digest): equality of
the digest is equality of every bit (every NaN counting as one NaN).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bwd_visit_scenes as vs  # noqa: E402
from parity_common import run_backend  # noqa: E402


def main(out=os.path.join(HERE, "bwd_visit.npz")):
    from online_lang_splatting_amd import _C, _lib
    dev = torch.device("cuda:0")
    ids, digs = [], []
    for tile in sorted(vs.IMAGES):
        for mode in (0, 1):
            for F in vs.F_VALUES:
                for N, (W, H), variant, bg in vs.cases(tile):
                    sc, kw, _ = vs.make(N, tile, F, W, H, variant, bg, plant_language=(mode == 1))
                    _, g = run_backend(_C, sc, dev, N, tile, mode, **{k: v.to(dev) for k, v in kw.items()})
                    torch.cuda.synchronize()
                    ids.append(vs.case_id(tile, mode, F, N, (W, H), variant, bg))
                    digs.append(vs.digest(g))
    np.savez_compressed(out, ids=np.array(ids), sha256=np.stack(digs))
    print(f"{len(ids)} cases -> {out} ({os.path.getsize(out)} bytes), library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main(*sys.argv[1:])
