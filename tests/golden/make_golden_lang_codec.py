"""Generates tests/golden/lang_codec.npz: the reference's OWN EncoderDecoderOnline (language/autoencoder/model.py:314-354)
driven through the statements of BackEnd.train_online_autoencoder (utils/slam_backend.py:266-323) on the CPU, in float64
("truth", *_f64) and float32 ("ref32", *_f32).  Runs ONLY in the authoring container (needs the reference checkout); the
committed .npz is data.

The module imports with lightning / lightning.pytorch (LightningModule = nn.Module), open_clip, torchvision(.models) and
eval.colormaps stubbed; nothing else of it is touched.

Cases: N = 1000 and N = 257 (no multiple of any block size) x seeds 0-3 (nn.Linear's default initialisation under
torch.manual_seed(seed)); features and the tie-row redraw as tests/lang_codec_ref.py describes (kept as int16 q).  Per case:
    params [2351] float32, q [N,32] int16, redrawn (rows the tie filter redrew)
    step 0:   grad0 [2351], codes_pre0 / codes_post0 (before / after the update)
    30 steps at lr = 1e-3:   loss [30,4] = {total, L1, 0.6 (1 - cos), mean cos} per step, params30 [2351], codes_post30
loss and grad0 in both precisions; of the others the float64 array and the float32 run's largest error (*_f32_maxerr).
The codes are kept for every 64th row only (the file stays small): the tests take the per-row truth from lang_codec_ref,
which tests/test_lang_codec_ref_golden.py pins to these arrays."""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OLSR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import lang_codec_ref as R  # noqa: E402

for name in ("lightning", "lightning.pytorch", "open_clip", "torchvision", "torchvision.models", "eval.colormaps"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["lightning.pytorch"].LightningModule = nn.Module
sys.modules["lightning"].pytorch = sys.modules["lightning.pytorch"]
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
sys.modules["eval.colormaps"].apply_pca_colormap = None

from language.autoencoder.model import EncoderDecoderOnline  # noqa: E402

LR, STEPS = 1e-3, 30


def reference_model(flat, dtype):
    m = EncoderDecoderOnline().to(dtype)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in R.STATE]
    m.load_state_dict({k: v.to(dtype) for k, v in R.unflatten(flat).items()})
    return m


def main():
    out = dict(lr=np.float64(LR), steps=np.int32(STEPS), tau=np.float64(R.TAU), row_stride=np.int32(R.CODE_ROW_STRIDE),
               state_names=np.array([k for k, _ in R.STATE]), state_shapes=np.array([list(s) + [0] * (2 - len(s)) for _, s in R.STATE]))
    for key, N, seed in R.golden_cases():
        flat, q, redrawn = R.make_case(N, seed)
        # the default initialisation is the reference module's own: same seed, same draws
        torch.manual_seed(seed)
        assert torch.equal(R.flatten(EncoderDecoderOnline().state_dict()), flat)
        x = R.unit(q)
        out[f"{key}_params"] = flat.numpy()
        out[f"{key}_q"] = q
        out[f"{key}_redrawn"] = np.int32(redrawn)
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            t = R.train(flat, x, LR, STEPS, dtype, model=reference_model(flat, dtype))
            sub = slice(None, None, R.CODE_ROW_STRIDE)
            out[f"{key}_loss_{tag}"] = t["loss"].numpy()
            out[f"{key}_grad0_{tag}"] = t["grad0"].numpy()
            if tag == "f32":   # of the float32 run the loss and the gradient are kept, of the rest only the error's size
                for name, a in (("codes_pre0", t["codes_pre0"][sub]), ("codes_post0", t["codes_post0"][sub]),
                                ("params30", t["params"]), ("codes_post30", t["codes_post"][sub])):
                    out[f"{key}_{name}_f32_maxerr"] = np.float64(np.abs(a.double().numpy() - out[f"{key}_{name}_f64"]).max())
                continue
            out[f"{key}_codes_pre0_{tag}"] = t["codes_pre0"][sub].numpy()
            out[f"{key}_codes_post0_{tag}"] = t["codes_post0"][sub].numpy()
            out[f"{key}_params30_{tag}"] = t["params"].numpy()
            out[f"{key}_codes_post30_{tag}"] = t["codes_post"][sub].numpy()
        e = np.abs(out[f"{key}_grad0_f32"].astype(np.float64) - out[f"{key}_grad0_f64"]).max()
        print(f"{key}: {redrawn} rows redrawn; gradient largest element {np.abs(out[f'{key}_grad0_f64']).max():.3e}, ref32 error "
              f"{e:.3e}; loss {out[f'{key}_loss_f64'][0, 0]:.6f} -> {out[f'{key}_loss_f64'][-1, 0]:.6f}, ref32 loss error after "
              f"{STEPS} steps {abs(float(out[f'{key}_loss_f32'][-1, 0]) - out[f'{key}_loss_f64'][-1, 0]):.3e}")
    path = os.path.join(HERE, "lang_codec.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
