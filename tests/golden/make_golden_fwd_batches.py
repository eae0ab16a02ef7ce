"""Records tests/golden/fwd_batches.npz: the images of the forward's two other accumulations (OLSR_FLAG_FWD_ACCUM_MFMA and
OLSR_FLAG_FWD_ACCUM_WEIGHT) on the scenes of tests/fwd_batch_scenes.py, as the build of the commit BEFORE those scenes existed
computes them.  tests/test_gpu_fwd_batches.py holds every later build to the same bits.  The default accumulation needs no
golden: the CPU oracle is its golden, bit for bit.

Run on a GPU, with that build selected:
    OLSR_LIB=/path/to/libolsr_of_that_commit.so OLSR_BINDING=ctypes python tests/golden/make_golden_fwd_batches.py

The fixture holds one SHA-256 per (tile, F, case, variant) over the fp32 bits of colour, language, depth and opacity
(fwd_batch_scenes.digest): equality of the digest is equality of every bit.
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

import fwd_batch_scenes as fs  # noqa: E402
from parity_common import run_forward  # noqa: E402


def main(out=os.path.join(HERE, "fwd_batches.npz")):
    from online_lang_splatting_amd import _C, _lib
    dev = torch.device("cuda:0")
    ids, digs = [], []
    for tile in fs.TILES:
        for F in fs.F_OTHER:
            for case in fs.cases(tile):
                sc, _ = fs.make(case, tile, F)
                for vname, flag in fs.ACCUM_VARIANTS:
                    _C.FLAGS = flag
                    try:
                        f, _ = run_forward(_C, sc, dev, tile, 0)
                        torch.cuda.synchronize()
                    finally:
                        _C.FLAGS = 0
                    ids.append(fs.case_id(tile, F, case, vname))
                    digs.append(fs.digest(f))
    np.savez_compressed(out, ids=np.array(ids), sha256=np.stack(digs))
    print(f"{len(ids)} cases -> {out} ({os.path.getsize(out)} bytes), library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main(*sys.argv[1:])
