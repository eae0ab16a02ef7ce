"""Generates tests/golden/keyframe_seed.npz from what the reference lets us import on the CPU (runs ONLY in the authoring
container, which holds the reference tree).  The committed .npz is data:
  rgb2sh_table      RGB2SH(torch.arange(256) / 255) (gaussian_splatting/utils/sh_utils.py:121), the 256 colours a byte image has
  opacity_half      inverse_sigmoid(0.5) (gaussian_splatting/utils/general_utils.py:20)
  pose{k}_R, _T     three poses and
  pose{k}_w2c       getWorld2View2(R, T) (gaussian_splatting/utils/graphics_utils.py:33), the matrix create_pcd_from_image_and_depth
                    hands Open3D as the extrinsic
Open3D is not installed here: the back-projection and the count rule of random_down_sample are not recorded."""
import math
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, REF)
from gaussian_splatting.utils.general_utils import inverse_sigmoid  # noqa: E402
from gaussian_splatting.utils.graphics_utils import getWorld2View2  # noqa: E402
from gaussian_splatting.utils.sh_utils import RGB2SH  # noqa: E402

out = {"rgb2sh_table": RGB2SH(torch.arange(256) / 255).numpy(),
       "opacity_half": inverse_sigmoid(0.5 * torch.ones(1, dtype=torch.float)).numpy()}
for k, (yaw, pitch, T) in enumerate([(0.0, 0.0, (0.0, 0.0, 0.0)), (25.0, -10.0, (0.4, -0.2, 1.3)), (-140.0, 33.0, (-2.5, 0.7, 0.1))]):
    a, b = math.radians(yaw), math.radians(pitch)
    Ry = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    R, t = (Rx @ Ry).contiguous(), torch.tensor(T)
    out[f"pose{k}_R"], out[f"pose{k}_T"] = R.numpy(), t.numpy()
    out[f"pose{k}_w2c"] = getWorld2View2(R, t).numpy()
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "keyframe_seed.npz"), **out)
print("wrote keyframe_seed.npz:", {k: v.shape for k, v in out.items()})
