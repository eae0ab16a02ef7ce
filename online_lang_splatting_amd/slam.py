"""The online SLAM session: RGB-D frames in, poses and a (language) Gaussian map out.

`OnlineSlam` joins the fused pieces of this package in the order the reference's FrontEnd.run (utils/slam_frontend.py:577-676,
:134-161 for the first frame) and BackEnd.run (utils/slam_backend.py:325-452 initialize_map, :499-767 map, :918-990 the
keyframe message) run them with `single_thread: True`: one process, one stream, tracking and mapping strictly one after the
other.  This module only sequences calls, like the reference's Python does; every number comes from libolsr.so.

    frame -> frontend.ingest_frame -> frontend.tracking_mask
    first frame:  GaussianMap.extend_from_rgbd(init=True) -> init_itr_num x MappingStep (one view, no exposure, no language)
                  with densify_and_prune / reset_opacity in its edit hook -> the frame enters the window
    later frames: PoseState.reset(previous estimate) -> tracking_itr_num x TrackingLoop.iteration -> KeyframeSelector.observe
    keyframe:     extend_from_rgbd(init=False) -> KeyframeWindow (pose_window views at half rates, exposures, nothing for the
                  first frame) -> language target -> mapping_itr_num x MappingStep(window + 2 rehearsal views, isotropic 10)
                  with densify_and_prune / reset_opacity_nonvisible in its edit hook -> the co-visibility prune of a full
                  window -> poses and visibilities handed back to the selector and the tracker

Hand-over rules after a map edit (DESIGN.md has the reasons): the lanes' workspaces follow the map's P before anything
renders; a keyframe's visibility in the selector is always n_touched > 0 of a render of the CURRENT map rows from the
keyframe's CURRENT pose (refreshed at the end of every keyframe's mapping, gathered through src_index when the prune drops
rows); the selector's and the trajectory's poses of the window's keyframes are the bundle adjustment's after every keyframe.

Stated deviations from the reference.  (1) The `prune=True` pass renders the window's views only (the reference also renders
two rehearsal views and runs a backward whose gradients it never uses when the prune happens; when the window is not full
they leak into the next optimiser step — that leak is not reproduced).  (2) The first frame's visibility is taken from a
render after the last initialisation step, not from that step's own render.  (3) Rehearsal views are rendered with a zero
exposure (MappingStep shares one exposure among the views outside the window).  (4) When tracking converges before its last
iteration the kept images are those of the pose after the converging step (TrackingLoop.render_final), one step of less than
1e-4 later than the reference's.  (5) Densification noise and the rehearsal draws come from one CPU torch.Generator seeded
with `Training.seed` (default 0): two runs are bit-identical.

OUT OF SCOPE: `single_thread: False` (tracking against a stale snapshot while the back end maps), the GUI packets,
pause / unpause, resuming a whole session from disk (the map alone resumes: GaussianMap.save_state / load_state), the .npy
language dumps and images of eval_rendering, LPIPS, datasets and image decoding, undistortion, and the language backbone
(its features arrive through `feature_fn`).

The end of the reference's run is here too: `save_gaussians` writes the map as the reference's point_cloud.ply
(map_io.py), `save_trajectory` the two JSON files of eval_ate."""
import json
import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

REQUIRED_KEYS = tuple(
    [f"Training.{k}" for k in (
        "init_itr_num", "init_gaussian_update", "init_gaussian_reset", "init_gaussian_th", "init_gaussian_extent",
        "tracking_itr_num", "mapping_itr_num", "gaussian_update_every", "gaussian_update_offset", "gaussian_th",
        "gaussian_extent", "gaussian_reset", "size_threshold", "kf_interval", "window_size", "pose_window", "edge_threshold",
        "rgb_boundary_threshold", "kf_translation", "kf_min_translation", "kf_overlap", "prune_mode", "use_gt_pose",
        "lr.cam_rot_delta", "lr.cam_trans_delta")] +
    [f"opt_params.{k}" for k in (
        "position_lr_init", "position_lr_final", "position_lr_max_steps", "feature_lr", "opacity_lr", "scaling_lr",
        "rotation_lr", "percent_dense", "lambda_dssim", "densify_grad_threshold", "densify_from_iter")] +
    [f"Dataset.{k}" for k in ("type", "pcd_downsample", "pcd_downsample_init", "point_size", "adaptive_pointsize")] +
    ["language.language_train"])
# read only when language.language_train is true
LANGUAGE_KEYS = ("language.single_stage_ae", "language.lang_code_size", "opt_params.language_lr")
# optional, with the reference's defaults: Training.alpha (get_loss_mapping_rgbd's 0.95), Training.seed,
# Training.spatial_lr_scale and Training.cameras_extent (slam.py: init_lr(6.0), cameras_extent = 6.0)
DEFAULTS = {"Training.alpha": 0.95, "Training.seed": 0, "Training.spatial_lr_scale": 6.0, "Training.cameras_extent": 6.0,
            "Training.kf_cutoff": 0.4}


def config_value(config: Dict, path: str):
    """config["A"]["b"]["c"] for path "A.b.c"; a missing key raises KeyError naming the whole path."""
    node = config
    for part in path.split("."):
        if not isinstance(node, dict) or part not in node:
            if path in DEFAULTS:
                return DEFAULTS[path]
            raise KeyError(path)
        node = node[part]
    return node


def parse_config(config: Dict) -> Dict:
    """The keys OnlineSlam consumes, flat ("Training.lr.cam_rot_delta" -> value).  Unknown keys are ignored."""
    if not isinstance(config, dict):
        raise TypeError("config must be a nested dict with the reference's YAML keys")
    flat = {k: config_value(config, k) for k in REQUIRED_KEYS + tuple(DEFAULTS)}
    if flat["language.language_train"]:
        flat.update({k: config_value(config, k) for k in LANGUAGE_KEYS})
    if flat["Training.prune_mode"] not in ("slam", "odometry"):
        raise ValueError("Training.prune_mode must be 'slam' or 'odometry'")
    return flat


def ate_rmse(est_w2c, gt_w2c) -> float:
    """eval_ate / evaluate_evo (utils/eval_utils.py:24-111) with correct_scale=False, on the host in float64: the camera
    centres of the inverted poses, a rigid Umeyama alignment (rotation and translation, no scale) of the estimate to the
    ground truth, the root mean square of the translation differences.  est_w2c, gt_w2c: [n,4,4] world-to-camera."""
    return ate_statistics(est_w2c, gt_w2c)["rmse"]


def ate_statistics(est_w2c, gt_w2c) -> Dict[str, float]:
    """evo's APE.get_all_statistics() of the translation part after ate_rmse's alignment: rmse, mean, median, std, min, max
    and sse of the per-pose distances (what evaluate_evo writes to stats_{label}.json)."""
    def centres(T):
        T = np.asarray(T.detach().cpu() if isinstance(T, torch.Tensor) else T, dtype=np.float64).reshape(-1, 4, 4)
        return np.stack([np.linalg.inv(t)[:3, 3] for t in T])
    x, y = centres(est_w2c), centres(gt_w2c)
    if x.shape != y.shape or x.shape[0] < 1:
        raise ValueError("ate_rmse: two trajectories of the same length, at least one pose")
    mx, my = x.mean(axis=0), y.mean(axis=0)
    cov = (y - my).T @ (x - mx) / x.shape[0]
    U, _, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    t = my - R @ mx
    err = (x @ R.T + t) - y
    sq = np.sum(err * err, axis=1)
    e = np.sqrt(sq)
    return dict(rmse=float(np.sqrt(np.mean(sq))), mean=float(np.mean(e)), median=float(np.median(e)), std=float(np.std(e)),
                min=float(np.min(e)), max=float(np.max(e)), sse=float(np.sum(sq)))


class OnlineSlam:
    """OnlineSlam(config, intrinsics, H, W, targets=None, feature_fn=None, lanes=1, device="cuda").

    config: the reference's YAML as a nested dict (REQUIRED_KEYS; a missing one raises KeyError with its dotted path).
    intrinsics = (fx, fy, cx, cy).  targets: an OnlineLanguageTargets or SingleStageTargets, or None.
    feature_fn(frame_idx, image [3,H,W]) -> a ready [F,h,w] code map (the labels_from_file path; works with targets=None), or
    what targets.add_keyframe takes (a tensor), or a tuple (method name, *arguments) for another add_keyframe* method of the
    targets object, e.g. ("add_keyframe_hr", hr_features).  With neither targets nor feature_fn, or with
    language.language_train false, the map has no language channel (F = 0).
    `events` is the ordered log of what ran: ("init", idx), ("track", idx, iterations), ("keyframe", idx, window),
    ("removed", kf), ("map", iteration_count, n_views), ("densify", iteration_count), ("reset_opacity", iteration_count),
    ("prune", P_before, P_after), ("language", kf).  GPU only."""

    def __init__(self, config: Dict, intrinsics: Sequence[float], H: int, W: int, targets=None,
                 feature_fn: Optional[Callable] = None, lanes: int = 1, device="cuda", capacity: Optional[int] = None):
        self.cfg = parse_config(config)
        c = self.cfg
        self.H, self.W = int(H), int(W)
        self.intrinsics = tuple(float(v) for v in intrinsics)
        if len(self.intrinsics) != 4:
            raise ValueError("intrinsics = (fx, fy, cx, cy)")
        self.targets, self.feature_fn, self.n_lanes = targets, feature_fn, int(lanes)
        self.language = bool(c["language.language_train"]) and (targets is not None or feature_fn is not None)
        self.F = int(c["language.lang_code_size"]) if self.language else 0
        self.two_stage = self.language and targets is not None and not bool(c["language.single_stage_ae"])
        self.mask_mode = "blocks" if c["Dataset.type"] == "replica" else "global"
        self.use_gt_pose = c["Training.use_gt_pose"] is True
        scale = float(c["Training.spatial_lr_scale"])
        self.position_schedule = (float(c["opt_params.position_lr_init"]) * scale, float(c["opt_params.position_lr_final"]) * scale,
                                  int(c["opt_params.position_lr_max_steps"]))
        feature_lr = float(c["opt_params.feature_lr"])
        self.lrs = dict(xyz=self.position_schedule[0], sh_dc=feature_lr, sh_rest=feature_lr / 20.0,
                        opacity=float(c["opt_params.opacity_lr"]), scale=float(c["opt_params.scaling_lr"]) * scale,
                        rotation=float(c["opt_params.rotation_lr"]),
                        language=float(c["opt_params.language_lr"]) if self.language else 0.0)
        extent = float(c["Training.cameras_extent"])
        self.init_extent = extent * float(c["Training.init_gaussian_extent"])
        self.map_extent = extent * float(c["Training.gaussian_extent"])
        self.capacity = int(capacity) if capacity is not None else max(600_000, 6 * self.W * self.H)
        self.device = torch.device(device)
        self.events: List[tuple] = []
        self._clear()

    # ---- state ---------------------------------------------------------------------------------------------------------
    def _clear(self):
        self.map = None
        self.lanes = None
        self.selector = None
        self.pose = None
        self.iteration_count = 0
        self.first_idx = None
        self.last_idx = None
        self.poses: Dict[int, torch.Tensor] = {}          # frame id -> estimated w2c [4,4] on the device
        self.keyframes: List[int] = []                    # every keyframe so far, oldest first
        self.kf_image: Dict[int, torch.Tensor] = {}
        self.kf_depth: Dict[int, torch.Tensor] = {}
        self.kf_exposure: Dict[int, torch.Tensor] = {}
        self.kf_lang: Dict[int, Optional[torch.Tensor]] = {}
        self._kf_camera: Dict[int, Dict] = {}             # cameras of keyframes outside the window (rehearsal views)
        self._xyz_lr = self.position_schedule[0]
        self.gen = torch.Generator().manual_seed(int(self.cfg["Training.seed"]))

    def reset(self):
        """Forget the map, the window and the trajectory; the next track() initialises again.  `events` is kept."""
        self._clear()

    def _setup_device(self):
        from .scene import projection_matrix2
        fx, fy, cx, cy = self.intrinsics
        dev = self.device
        self.proj = projection_matrix2(0.01, 100.0, cx, cy, fx, fy, self.W, self.H).transpose(0, 1).contiguous().to(dev)
        self.tanfovx, self.tanfovy = self.W / (2.0 * fx), self.H / (2.0 * fy)
        self.bg = torch.zeros(3, dtype=torch.float32, device=dev)

    def _sync_lanes(self):
        """The tracker's and the mapper's workspaces follow the map's rows."""
        if self.map.P == 0:
            raise RuntimeError("OnlineSlam: the map has no Gaussian left (a reset or a prune threshold the configured iteration "
                               "counts cannot recover from)")
        if self.lanes.P != self.map.P:
            self.lanes.resize(self.map.P)

    def _scene(self) -> Dict:
        from . import _abi
        return dict(self.map.params, bg=self.bg, activations=_abi.ACT_ALL)

    def _pose_state(self, T):
        from .slam_iterations import PoseState
        c = self.cfg
        return PoseState(T, self.proj, self.tanfovx, self.tanfovy, lr_rot=float(c["Training.lr.cam_rot_delta"]),
                         lr_trans=float(c["Training.lr.cam_trans_delta"]), lr_exposure=0.01)

    def _forward(self, camera: Dict) -> Dict:
        """One plain forward of the current map from `camera` on the first lane's workspace (images in ws.out)."""
        self._sync_lanes()
        ws = self.lanes.lanes[0][0]
        ws.tile_order = self._tile_order
        ws.depth_order_carry = None
        ws.set_scene(sh_degree=0, **camera, **self._scene())
        return ws.forward()

    def _draw_noise(self):
        return torch.randn(self.map.P, 2, 3, generator=self.gen).to(self.device)

    # ---- the public face -----------------------------------------------------------------------------------------------
    def track(self, frame_idx: int, rgb_u8: torch.Tensor, depth: torch.Tensor, depth_scale: float,
              gt_w2c: Optional[torch.Tensor] = None) -> Dict:
        """One frame (FrontEnd.run, utils/slam_frontend.py:577-676).  rgb_u8 uint8 [H,W,3] and depth uint16 / float32 [H,W] on
        the device (frontend.ingest_frame's inputs); gt_w2c [4,4]: the first frame's pose (identity when None) and, with
        Training.use_gt_pose, every frame's.  -> dict(w2c [4,4] a copy, is_keyframe, window, converged, iterations)."""
        from .frontend import ingest_frame, tracking_mask
        frame_idx = int(frame_idx)
        if tuple(rgb_u8.shape) != (self.H, self.W, 3):
            raise ValueError(f"track: rgb_u8 must be [H,W,3] = [{self.H},{self.W},3]")
        image, gt_depth = ingest_frame(rgb_u8, depth, depth_scale)
        mask = tracking_mask(image, float(self.cfg["Training.edge_threshold"]), self.mask_mode)
        if gt_w2c is not None:
            gt_w2c = gt_w2c.detach().to(device=self.device, dtype=torch.float32).reshape(4, 4).contiguous()
        if self.map is None:
            return self._initialize(frame_idx, image, gt_depth, gt_w2c)
        if self.use_gt_pose and gt_w2c is None:
            raise ValueError("track: Training.use_gt_pose needs gt_w2c for every frame")
        from .slam_iterations import TrackingLoop
        c = self.cfg
        self._sync_lanes()
        ws = self.lanes.lanes[0][0]
        ws.tile_order = self._tile_order
        ws.depth_order_carry = None
        self.pose.reset(self.poses[self.last_idx])
        loop = TrackingLoop(ws, self._scene(), 0, self.pose, image, gt_depth, mask, alpha=float(c["Training.alpha"]),
                            rgb_boundary_threshold=float(c["Training.rgb_boundary_threshold"]))
        n = int(c["Training.tracking_itr_num"])
        if self.use_gt_pose:
            n = min(n, 51)   # converged = (tracking_itr == 50), utils/slam_frontend.py:238-240
        iterations, converged = 0, False
        for k in range(n):
            last = k == n - 1
            flag = loop.iteration(read_convergence=not self.use_gt_pose, write_images=last)
            iterations += 1
            if self.use_gt_pose:
                self.pose.T_w2c.copy_(gt_w2c)
                self.pose._call(None, None)   # the matrices of the ground-truth pose; the optimiser state is kept
                converged = k == 50
            elif flag:
                converged = True
                if not last:
                    loop.render_final()
                break
        if n == 0:
            if self.use_gt_pose:
                self.pose.T_w2c.copy_(gt_w2c)
                self.pose._call(None, None)
            loop.render_final()
        self.events.append(("track", frame_idx, iterations))
        w2c = self.pose.T_w2c.clone()
        self.poses[frame_idx] = w2c
        self.last_idx = frame_idx
        create, window, removed, _ = self.selector.observe(frame_idx, ws.out["n_touched"], self.pose, ws.out["depth"],
                                                           ws.out["opacity"])
        if create:
            self.events.append(("keyframe", frame_idx, tuple(window)))
            for kf in removed:
                self.events.append(("removed", kf))
            self._keyframe(frame_idx, image, gt_depth, window)
        return dict(w2c=self.poses[frame_idx].clone(), is_keyframe=bool(create), window=list(self.selector.window),
                    converged=bool(converged), iterations=iterations)

    def trajectory(self):
        """-> (frame ids, w2c [n,4,4] on the device): every frame's estimate; a keyframe's is the bundle adjustment's."""
        ids = sorted(self.poses)
        return ids, torch.stack([self.poses[i] for i in ids]) if ids else torch.zeros(0, 4, 4, device=self.device)

    def save_gaussians(self, save_dir, iteration=None, final=False):
        """save_gaussians (utils/eval_utils.py:202-211): the map as `point_cloud/final/point_cloud.ply` or
        `point_cloud/iteration_{iteration}/point_cloud.ply` under save_dir (GaussianMap.save_ply: packed on the device,
        written through a temporary file).  save_dir=None returns without writing.  -> the file's path or None."""
        if save_dir is None:
            return None
        if self.map is None:
            raise RuntimeError("save_gaussians: no frame has been tracked yet")
        if not final and iteration is None:
            raise ValueError("save_gaussians: an iteration, or final=True")
        sub = "final" if final else "iteration_{}".format(str(iteration))
        path = os.path.join(os.fspath(save_dir), "point_cloud", sub, "point_cloud.ply")
        self.map.save_ply(path)
        return path

    def save_trajectory(self, save_dir, gt_w2c, iterations=None, final=False) -> float:
        """eval_ate (utils/eval_utils.py:67-111) over the keyframes so far: `plot/trj_{label}.json` with trj_id, trj_est and
        trj_gt (camera-to-world 4x4 lists: the float64 inverses of the float32 world-to-camera poses) and
        `plot/stats_{label}.json` with evo's rmse, mean, median, std, min, max and sse (ate_statistics), label = "final" or
        the four-digit `iterations`.  gt_w2c: a mapping frame id -> [4,4] world-to-camera.  Host only.  -> the RMSE."""
        if not final and iterations is None:
            raise ValueError("save_trajectory: iterations, or final=True")
        if not self.keyframes:
            raise RuntimeError("save_trajectory: no keyframe yet")

        def f64(T):
            T = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else np.asarray(T)
            return T.astype(np.float64).reshape(4, 4)
        ids = [int(k) for k in self.keyframes]
        est, gt = [f64(self.poses[k]) for k in ids], [f64(gt_w2c[k]) for k in ids]
        trj = dict(trj_id=ids, trj_est=[np.linalg.inv(T).tolist() for T in est], trj_gt=[np.linalg.inv(T).tolist() for T in gt])
        stats = ate_statistics(np.stack(est), np.stack(gt))
        plot_dir = os.path.join(os.fspath(save_dir), "plot")
        os.makedirs(plot_dir, exist_ok=True)
        label = "final" if final else "{:04}".format(int(iterations))
        for name, data in ((f"trj_{label}.json", trj), (f"stats_{label}.json", stats)):
            tmp = os.path.join(plot_dir, name + ".tmp")
            with open(tmp, "w", encoding="utf-8") as f:
                json.dump(data, f, indent=4)
            os.replace(tmp, os.path.join(plot_dir, name))
        return stats["rmse"]

    def render(self, w2c: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The map seen from a world-to-camera pose: copies of color [3,H,W], depth, opacity [1,H,W], language [F,H,W],
        radii and n_touched [P]."""
        if self.map is None:
            raise RuntimeError("render: no frame has been tracked yet")
        T = w2c.detach().to(device=self.device, dtype=torch.float32).reshape(4, 4)
        out = self._forward(self._pose_state(T).camera())
        return {k: v.clone() for k, v in out.items()}

    def mapping_loss(self, kf: int) -> torch.Tensor:
        """The mapping loss [4] = {total, rgb, depth, language} of keyframe `kf` as the map renders it now from the
        keyframe's current pose and exposure (losses.mapping_loss); stays on the device."""
        from . import losses
        out = self._forward(self._pose_state(self.poses[kf]).camera())
        target = self.kf_lang.get(kf) if self.F > 0 else None
        lo = losses.mapping_loss(out["color"], out["depth"], out["language"] if target is not None else None, self.kf_image[kf],
                                 self.kf_depth[kf], target, self.kf_exposure[kf],
                                 alpha=float(self.cfg["Training.alpha"]),
                                 rgb_boundary_threshold=float(self.cfg["Training.rgb_boundary_threshold"]))
        return lo["loss"].clone()

    def finish(self, refine_iters: int = 0):
        """The end of the run: BackEnd.color_refinement (utils/slam_backend.py:769-819) for `refine_iters` iterations through
        RefinementStep, each on a keyframe drawn from the session's generator.  -> the last loss [4] or None."""
        if self.map is None or int(refine_iters) <= 0:
            return None
        from .slam_iterations import RefinementStep
        self._sync_lanes()
        kfs = list(self.keyframes)
        cams = [self._pose_state(self.poses[k]).camera() for k in kfs]
        rs = RefinementStep(self.lanes, None, self.bg, 0, cams, [self.kf_image[k] for k in kfs], dict(self.lrs),
                            lambda_dssim=float(self.cfg["opt_params.lambda_dssim"]), position_schedule=self.position_schedule,
                            view_ids=kfs, gaussian_map=self.map)
        views = torch.randint(0, len(kfs), (int(refine_iters),), generator=self.gen).tolist()
        loss = rs.run(int(refine_iters), views=views)
        self._sync_lanes()
        return loss

    # ---- the first frame: FrontEnd.initialize + BackEnd.initialize_map ---------------------------------------------------
    def _initialize(self, idx, image, gt_depth, gt_w2c):
        from .frame_shard import FrameLanes
        from .frontend import KeyframeSelector
        from .gaussian_map import GaussianMap
        from .slam_iterations import MappingStep, OnlineLanguageTargets
        c = self.cfg
        dev = self.device
        self._setup_device()
        T = gt_w2c if gt_w2c is not None else torch.eye(4, dtype=torch.float32, device=dev)
        self.first_idx = self.last_idx = idx
        self.events.append(("init", idx))
        f32 = dict(dtype=torch.float32, device=dev)
        self.map = GaussianMap(torch.zeros(0, 3, **f32), torch.zeros(0, 1, 3, **f32), torch.zeros(0, 1, **f32),
                               torch.zeros(0, 3, **f32), torch.zeros(0, 4, **f32),
                               torch.zeros(0, self.F, **f32) if self.F else None, self.lrs,
                               percent_dense=float(c["opt_params.percent_dense"]), device=dev)
        self._seed(idx, image, gt_depth, T, None, init=True)
        if self.map.P == 0:
            raise RuntimeError("track: the first frame yields no Gaussian (no valid depth?)")
        self.lanes = FrameLanes(self.n_lanes, self.map.P, self.W, self.H, self.F, 1, self.capacity, dev)
        self._tile_order = self.lanes.lanes[0][0].tile_order.clone()
        self.pose = self._pose_state(T)
        self.poses[idx] = T.clone()
        self.keyframes = [idx]
        self.kf_image[idx], self.kf_depth[idx] = image, gt_depth
        self.kf_exposure[idx] = torch.zeros(2, **f32)
        camera = self.pose.camera()
        feats = None
        if self.two_stage and isinstance(self.targets, OnlineLanguageTargets):
            feats = self.feature_fn(idx, image)
        state = {"k": 0}

        def hook(step, total):
            k = state["k"]
            if k % int(c["Training.init_gaussian_update"]) == 0:
                self.map.densify_and_prune(float(c["opt_params.densify_grad_threshold"]), float(c["Training.init_gaussian_th"]),
                                           self.init_extent, None, z=self._draw_noise())
                self.events.append(("densify", self.iteration_count))
            if self.iteration_count in (int(c["Training.init_gaussian_reset"]), int(c["opt_params.densify_from_iter"])):
                self.map.reset_opacity()
                self.events.append(("reset_opacity", self.iteration_count))
            return None

        ms = MappingStep(self.lanes, None, self.bg, 0, [camera], [(image, gt_depth, None)], dict(self.lrs), exposure=None,
                         fused_loss=True, view_ids=[idx], gaussian_map=self.map, edit_hook=hook)
        for k in range(int(c["Training.init_itr_num"])):
            self.iteration_count += 1
            state["k"] = k
            self.events.append(("map", self.iteration_count, 1))
            if feats is not None and isinstance(feats, torch.Tensor) and k % 5 == 0:
                self.targets.codec.train_step(feats, 1e-3, codes=None)   # the online autoencoder's step of initialize_map
            ms.iteration()
        self.selector = KeyframeSelector(int(c["Training.window_size"]), int(c["Training.kf_interval"]),
                                         float(c["Training.kf_translation"]), float(c["Training.kf_min_translation"]),
                                         float(c["Training.kf_overlap"]), kf_cutoff=float(c["Training.kf_cutoff"]),
                                         single_thread=True)
        out = self._forward(camera)
        self.selector.add_keyframe(idx, T, out["n_touched"] > 0)
        return dict(w2c=T.clone(), is_keyframe=True, window=list(self.selector.window), converged=True, iterations=0)

    def _seed(self, idx, image, gt_depth, T, exposure, init):
        c = self.cfg
        return self.map.extend_from_rgbd(image, gt_depth, T.contiguous(), self.intrinsics, idx, init=init,
                                         downsample=int(c["Dataset.pcd_downsample_init" if init else "Dataset.pcd_downsample"]),
                                         exposure=exposure, rgb_boundary_threshold=float(c["Training.rgb_boundary_threshold"]),
                                         point_size=float(c["Dataset.point_size"]),
                                         adaptive_pointsize=bool(c["Dataset.adaptive_pointsize"]))

    # ---- a keyframe: the back end's "keyframe" message -------------------------------------------------------------------
    def _language_target(self, kf):
        """A window view's language target, made the first time the view is mapped (utils/slam_backend.py:535-576)."""
        if not self.language or kf in self.kf_lang:
            return
        out = self.feature_fn(kf, self.kf_image[kf]) if self.feature_fn is not None else None
        if out is None:
            self.kf_lang[kf] = None
            return
        if self.targets is None:
            if not (isinstance(out, torch.Tensor) and out.dim() == 3 and out.shape[0] == self.F):
                raise ValueError(f"feature_fn must return a [F,h,w] = [{self.F},h,w] code map when there is no targets object")
            target = out.detach().to(device=self.device, dtype=torch.float32).contiguous()
        elif isinstance(out, (tuple, list)):
            target = getattr(self.targets, out[0])(kf, *out[1:])
        else:
            target = self.targets.add_keyframe(kf, out)
        self.kf_lang[kf] = target
        self.events.append(("language", kf))

    def _keyframe(self, idx, image, gt_depth, window):
        from .slam_iterations import KeyframeWindow, MappingStep, OnlineLanguageTargets, position_lr
        c = self.cfg
        dev = self.device
        self.keyframes.append(idx)
        self.kf_image[idx], self.kf_depth[idx] = image, gt_depth
        self.kf_exposure[idx] = self.pose.exposure.clone()
        self._seed(idx, image, gt_depth, self.poses[idx], self.kf_exposure[idx], init=False)
        self._sync_lanes()
        window = [int(k) for k in window]
        in_window = set(window)
        pose_window = 0 if self.use_gt_pose else int(c["Training.pose_window"])
        win = KeyframeWindow([self.poses[k] for k in window], window, self.proj, self.tanfovx, self.tanfovy,
                             exposures=[self.kf_exposure[k] for k in window], pose_window=pose_window,
                             frozen_ids=(self.first_idx,), lr_rot=0.5 * float(c["Training.lr.cam_rot_delta"]),
                             lr_trans=0.5 * float(c["Training.lr.cam_trans_delta"]), lr_exposure=0.01)
        for k in window:
            self._language_target(k)
        rest = [k for k in self.keyframes if k not in in_window]
        for k in rest:
            if k not in self._kf_camera:
                self._kf_camera[k] = self._pose_state(self.poses[k]).camera()
        lang = (lambda k: self.kf_lang.get(k)) if self.F > 0 else (lambda k: None)
        online = self.two_stage and isinstance(self.targets, OnlineLanguageTargets)

        def hook(step, total):
            n = self.iteration_count
            step.lrs["xyz"] = self._xyz_lr
            if n % int(c["Training.gaussian_update_every"]) == int(c["Training.gaussian_update_offset"]):
                self.map.densify_and_prune(float(c["opt_params.densify_grad_threshold"]), float(c["Training.gaussian_th"]),
                                           self.map_extent, c["Training.size_threshold"], z=self._draw_noise())
                self.events.append(("densify", n))
            elif n % int(c["Training.gaussian_reset"]) == 0:
                self.map.reset_opacity_nonvisible([step.visibility[v] for v in step.view_ids])
                self.events.append(("reset_opacity", n))
            return None

        ms = MappingStep(self.lanes, None, self.bg, 0, [], [], dict(self.lrs), exposure=torch.zeros(2, device=dev),
                         fused_loss=True, view_ids=list(window), gaussian_map=self.map, edit_hook=hook,
                         record_visibility=True, window=win, isotropic_weight=10.0)
        for _ in range(int(c["Training.mapping_itr_num"])):
            self.iteration_count += 1
            picks = [rest[j] for j in torch.randperm(len(rest), generator=self.gen)[:2].tolist()]
            views = window + picks
            ms.cameras = [self._kf_camera[k] for k in picks]
            ms.view_ids = views
            ms.targets = [(self.kf_image[k], self.kf_depth[k], lang(k)) for k in views]
            self.events.append(("map", self.iteration_count, len(views)))
            if online and picks:
                self.targets.rehearse(picks)
            ms.iteration()
            self._xyz_lr = position_lr(self.iteration_count, *self.position_schedule)   # update_learning_rate(iteration_count)
        # the prune=True pass: every window view's visibility on the map as it is now, the co-visibility prune of a full window
        self.iteration_count += 1
        self._sync_lanes()
        vis = {k: (self._forward(win.camera(v))["n_touched"] > 0) for v, k in enumerate(window)}
        if len(window) == int(c["Training.window_size"]):
            before = self.map.P
            src = self.map.covisibility_prune([vis[k] for k in window], window, mode=c["Training.prune_mode"])
            self._sync_lanes()
            keep = src.long()
            vis = {k: v[keep] for k, v in vis.items()}
            self.events.append(("prune", before, self.map.P))
        # hand-over: the bundle adjustment's poses and exposures, and the surviving visibilities, to the front end
        for v, k in enumerate(window):
            self.poses[k] = win.T_w2c(v).clone()
            self.kf_exposure[k] = win.exposure(v).clone()
            self.selector.poses[k] = self.poses[k].reshape(16).clone()
            self.selector.set_visibility(k, vis[k])
        for k in list(self._kf_camera):
            if k in in_window:
                del self._kf_camera[k]
