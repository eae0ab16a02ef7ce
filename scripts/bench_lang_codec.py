"""Times the online language autoencoder on the GPU; prints one JSON line and writes profiles/lang_codec_bench.json.

(a) one training step on a keyframe's N = 36 864 feature rows: olsr_lang_ae_train_step (two launches) against the same
    step in torch ops on the same GPU — the body of the reference's train_online_autoencoder restated on torch.nn modules with
    torch.optim.Adam (tests/lang_codec_ref.py), including its loss.item() host read;
(b) olsr_lang_ae_encode (the [15,192,192] language target) and olsr_lang_ae_decode;
(c) a 12-view MappingStep.iteration on the room map (500 k Gaussians, 1200x680, F = 15) alone, followed by two rehearsal steps
    of the fused codec, and followed by two rehearsal steps in torch ops (what the reference adds to every mapping iteration).
Medians over `--reps` repetitions (default 60), each between its own pair of device events, after `--warmup` warm-up ones.
Required, not hoped for: the fused step's whole range over the repetitions lies below the torch-op step's range.
usage: bench_lang_codec.py [--reps N] [--warmup N] [--P N] [--no-mapping] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lang_codec_ref as R  # noqa: E402  (the torch restatement the tests hold the kernels to)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--P", type=int, default=500_000)
ap.add_argument("--no-mapping", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lang_codec_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lang_codec.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402

dev = torch.device("cuda:0")
N, LR = 192 * 192, 1e-4


def stats_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}


class TorchOpsStep:
    """train_online_autoencoder in torch ops on the GPU, float32."""

    def __init__(self, flat):
        self.model = R.codec_from(flat, torch.float32).to(dev)
        self.opt = torch.optim.Adam(self.model.parameters(), lr=LR)

    def __call__(self, x, host_read=True):
        self.model.train()
        self.opt.zero_grad()
        codes, terms = R.loss_terms(self.model, x)
        terms[0].backward()
        self.opt.step()
        return (terms[0].item() if host_read else terms[0]), codes.detach()


flat = R.initial_params(0)
g = torch.Generator().manual_seed(0)
feats = [R.unit(R.draw_q(N, g)).to(dev) for _ in range(3)]
codec = OnlineLanguageCodec(dev, seed=0)
codec.load_state_dict(R.unflatten(flat))
torch_step = TorchOpsStep(flat)
out = {"what": "online language autoencoder: train step, encode, mapping iteration with rehearsal", "N": N, "lr": LR,
       "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
out["train_step_fused"] = stats_ms(lambda: codec.train_step(feats[0], LR, codes="pre", layout="channels"), args.reps, args.warmup)
out["train_step_fused_no_codes"] = stats_ms(lambda: codec.train_step(feats[0], LR, codes=None), args.reps, args.warmup)
out["train_step_torch_ops"] = stats_ms(lambda: torch_step(feats[0]), args.reps, args.warmup)
out["train_step_torch_ops_no_host_read"] = stats_ms(lambda: torch_step(feats[0], host_read=False), args.reps, args.warmup)
out["encode"] = stats_ms(lambda: codec.encode(feats[0], "channels"), args.reps, args.warmup)
enc = codec.encode(feats[0]).clone()
out["decode"] = stats_ms(lambda: codec.decode(enc), args.reps, args.warmup)
out["train_step_speedup"] = round(out["train_step_torch_ops"]["ms_median"] / out["train_step_fused"]["ms_median"], 2)
out["ranges_disjoint"] = out["train_step_fused"]["ms_max"] < out["train_step_torch_ops"]["ms_min"]
# what the step must move at least: the features once, the codes once
out["train_step_algorithmic_bytes"] = N * 32 * 4 + N * 15 * 4

if not args.no_mapping:
    import bench  # noqa: E402
    from online_lang_splatting_amd import _abi  # noqa: E402
    from online_lang_splatting_amd.frame_shard import FrameLanes  # noqa: E402
    from online_lang_splatting_amd.scene import make_room_scene  # noqa: E402
    from online_lang_splatting_amd.slam_iterations import MappingStep, OnlineLanguageTargets  # noqa: E402
    W, H, Fch = 1200, 680, 15
    rs = make_room_scene(args.P, W, H, Fch, views=10, random_views=2, seed=3)
    sc, cams = rs.scene, rs.cameras
    M = sc.shs.shape[1]
    g_dev, _ = bench.device_inputs(sc, cams[0], dev)
    camd = [bench.device_inputs(sc, c, dev)[1] for c in cams]
    R0 = max(bench._sized_capacity(Fch, g_dev, c, H, W, 0, dev, (15, _abi.BWD_REFERENCE, _abi.BINNING_ELLIPSE)) for c in camd)
    lanes = FrameLanes(4, sc.P, W, H, Fch, M, int(1.5 * R0) + (1 << 16), dev)
    params = dict(means3D=g_dev["means3D"].clone(), shs=g_dev["shs"].clone(),
                  opacities=torch.logit(g_dev["opacities"].clamp(1e-4, 1 - 1e-4)).contiguous(),
                  scales=torch.log(g_dev["scales"]).contiguous(), rotations=g_dev["rotations"].clone(),
                  language=g_dev["language"].clone())
    lrs = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)
    # the language targets come from the codec: three keyframes' features, every view takes one of them
    lt = OnlineLanguageTargets(codec, lr=LR)
    for v in range(3):
        lt.add_keyframe(v, feats[v])
    targets = [(a, b, lt.targets[v % 3]) for v, (a, b, _) in enumerate(rs.targets)]
    stp = MappingStep(lanes, params, g_dev["bg"], 0, camd, targets, lrs, exposure=torch.zeros(2, device=dev), fused_loss=True)

    def with_fused():
        stp.iteration()
        lt.rehearse([1, 2])

    def with_torch_ops():
        stp.iteration()
        torch_step(feats[1])
        torch_step(feats[2])
    warm = max(args.warmup, 8)
    res = {"P": sc.P, "views": len(camd), "lanes": 4}
    res["iteration"] = stats_ms(stp.iteration, args.reps, warm)
    res["iteration_plus_2_fused_rehearsals"] = stats_ms(with_fused, args.reps, warm)
    res["iteration_plus_2_torch_op_rehearsals"] = stats_ms(with_torch_ops, args.reps, warm)
    it = res["iteration"]["ms_median"]
    res["fused_rehearsal_share_of_iteration"] = round((res["iteration_plus_2_fused_rehearsals"]["ms_median"] - it) / it, 4)
    res["torch_op_rehearsal_share_of_iteration"] = round((res["iteration_plus_2_torch_op_rehearsals"]["ms_median"] - it) / it, 4)
    out["mapping_iteration_room"] = res

line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
if not out["ranges_disjoint"]:
    raise SystemExit("the fused train step's range over the repetitions does not lie below the torch-op step's range")
