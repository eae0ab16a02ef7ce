"""Records tests/golden/bwd_batches.npz: the backward's gradients on the scenes of tests/bwd_batch_scenes.py, as the build of
the commit BEFORE the staging batch became a template parameter of render_bwd_kernel computes them (one 128-entry batch for
every instantiation).  tests/test_gpu_bwd_batches.py holds every later build to the same bits.

Run on a GPU, with that build selected:
    OLSR_LIB=/path/to/libolsr_of_that_commit.so OLSR_BINDING=ctypes python tests/golden/make_golden_bwd_batches.py

The full gradients of the 480 cases are 8 MB of floats, so the fixture holds one SHA-256 per case over the fp32 bits of
every gradient tensor (bwd_batch_scenes.digest): equality of the digest is equality of every bit.
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

import bwd_batch_scenes as bs  # noqa: E402
from parity_common import run_backend  # noqa: E402


def main(out=os.path.join(HERE, "bwd_batches.npz")):
    from online_lang_splatting_amd import _C, _lib
    dev = torch.device("cuda:0")
    ids, digs = [], []
    for tile in bs.TILES:
        for mode in (0, 1):
            for F in bs.F_VALUES:
                for N, lower, bg in bs.cases(tile, F):
                    sc, _ = bs.make(N, tile, F, lower, bg)
                    _, g = run_backend(_C, sc, dev, N, tile, mode)
                    torch.cuda.synchronize()
                    ids.append(bs.case_id(tile, mode, F, N, lower, bg))
                    digs.append(bs.digest(g))
    np.savez_compressed(out, ids=np.array(ids), sha256=np.stack(digs))
    print(f"{len(ids)} cases -> {out} ({os.path.getsize(out)} bytes), library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main(*sys.argv[1:])
