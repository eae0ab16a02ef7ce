"""The two loops the reference's SLAM system spends its GPU time in, written over this library's sync-free entry
points ("the callers either side of the path").  They are the measurable substitute
for BASELINE.json configs[3] (the Replica `slam.py` loop, which needs data, checkpoints and front-end dependencies this
image lacks) and are what `bench.py` reports under `config4_substitute`.

TrackingLoop   front end, utils/slam_frontend.py:tracking() (:160-275): up to 100 DEPENDENT iterations per frame of
               render -> get_loss_tracking (utils/slam_utils.py:92-121, no language term) -> backward to the camera pose
               only -> Adam on (cam_rot_delta, cam_trans_delta) -> update_pose (utils/pose_utils.py:update_pose).
               Iterations depend on each other through the pose: this is the single-frame LATENCY of the path.
MappingStep    back end, utils/slam_backend.py:map() (:499-760): 12 views of the same Gaussians (10 window keyframes +
               2 random), mapping loss incl. the language L1 (:579-597), gradients summed over the views, ONE Adam step.
KeyframeWindow back end, the bundle adjustment of map(): `keyframe_optimizers` (:933-980) — poses of the first pose_window
               window keyframes at half the tracking rates, exposures of every window keyframe, nothing for frame 0 — stepped
               once per mapping iteration with update_pose (:756-765), in ONE launch (olsr_window_pose_step).

OnlineLanguageTargets  back end, the language targets of map(): train_online_autoencoder (:266-323) once per new keyframe
               (:562-576, the returned codes are the keyframe's gt_lang_feat) and once per rehearsal view (:640-648).

RefinementStep back end, utils/slam_backend.py:color_refinement() (:769-819): 26 000 DEPENDENT iterations of one random
               keyframe -> (1 - lambda) L1 + lambda (1 - SSIM) on the colour image -> backward -> Adam on every group ->
               position learning-rate decay.  No densification, pruning or pose update.

Everything numerical happens in libolsr.so (olsr_forward_async, olsr_tracking_loss / olsr_mapping_loss /
olsr_refinement_loss, olsr_lang_ae_train_step, olsr_backward, olsr_pose_step, olsr_adam_step); this module only sequences the calls, like the
reference's Python does.
"""
import ctypes as C
import math
import random
from typing import Callable, Dict, Optional, Sequence

import torch

from . import _abi, losses
from ._host import stream_ptr
from ._lib import OlsrError, check, lib
from .frame_shard import FrameLanes, FusedAdam, GradLayout, RasterWorkspace


class PoseState:
    """Camera pose + the pose optimiser of one tracked frame, resident on the GPU and advanced by ONE kernel per
    iteration (olsr_pose_step): Adam on the six pose increments (torch.optim.Adam's arithmetic, lr per group as in
    utils/slam_frontend.py:170-196), new_w2c = SE3_exp(tau) @ T_w2c (utils/pose_utils.py:61-94), then the matrices the
    rasterizer consumes — world_view_transform = W2C^T, full_proj_transform = W2C^T P^T, camera_center
    (utils/camera_utils.py:103-117) — and the reference's convergence test |tau| < 1e-4."""

    def __init__(self, T_w2c: torch.Tensor, projection_matrix: torch.Tensor, tanfovx: float, tanfovy: float,
                 lr_rot=0.003, lr_trans=0.001, lr_exposure=0.01, betas=(0.9, 0.999), eps=1e-8,
                 converged_threshold=1e-4, optimise_exposure=True, device_step_count=False):
        """device_step_count: the Adam step number lives on the device (status[1]) instead of in the launch arguments —
        every iteration is then the same sequence of launches and can be replayed from a HIP graph (TrackingLoop.capture)."""
        dev = T_w2c.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.device = dev
        self.tanfovx, self.tanfovy = float(tanfovx), float(tanfovy)
        self.proj = projection_matrix.to(**f32).contiguous()  # P^T, what the callers hold
        self.state = torch.zeros(80, **f32)                    # layout: olsr_pose_step, include/olsr.h
        self.T_w2c = self.state[0:16].view(4, 4)
        self.viewmatrix = self.state[16:32].view(4, 4)
        self.projmatrix = self.state[32:48].view(4, 4)
        self.campos = self.state[48:51]
        self.last_tau = self.state[64:70]
        self.exposure = self.state[70:72]
        self.status = torch.zeros(2, dtype=torch.int32, device=dev)  # {converged flag, steps done}
        self.optimise_exposure = optimise_exposure
        self.device_step_count = device_step_count
        self.hp = _abi.OlsrPoseParams(lr_rot=lr_rot, lr_trans=lr_trans, lr_exposure=lr_exposure, beta1=betas[0],
                                      beta2=betas[1], eps=eps, converged_threshold=converged_threshold, step=0)
        self.reset(T_w2c)

    def reset(self, T_w2c, exposure=(0.0, 0.0)):
        """New frame: pose prior, fresh optimiser state (the reference builds a new Adam per tracked frame)."""
        T = T_w2c.detach().to(self.state).clone()
        self.state.zero_()
        self.T_w2c.copy_(T)
        self.exposure.copy_(torch.tensor(exposure, dtype=torch.float32))
        self.status.zero_()
        self.hp.step = 0
        self._call(None, None)  # the matrices of the start pose (no gradient: no step)

    def _call(self, dL_dtau_sum, dL_dexposure, frame_status=None):
        check(lib().olsr_pose_step_gated(C.byref(self.hp), dL_dtau_sum.data_ptr() if dL_dtau_sum is not None else None,
                                         dL_dexposure.data_ptr() if dL_dexposure is not None else None,
                                         self.proj.data_ptr(), self.state.data_ptr(), self.status.data_ptr(),
                                         frame_status.data_ptr() if frame_status is not None else None,
                                         stream_ptr(self.device)))

    def step(self, dL_dtau_sum: torch.Tensor, dL_dexposure: Optional[torch.Tensor] = None,
             frame_status: Optional[torch.Tensor] = None):
        """dL_dtau_sum: device float[6] = [rho | theta] as olsr_backward leaves it; dL_dexposure: device float[2] from
        olsr_tracking_loss (ignored unless optimise_exposure); frame_status: the forward's device int32[2] {R, status} —
        the step is skipped on the device when that frame was not usable (olsr_pose_step_gated; the step count must then
        live on the device too)."""
        if frame_status is not None and not self.device_step_count:
            raise ValueError("a gated pose step needs PoseState(device_step_count=True): the host cannot know whether it counted")
        if not self.device_step_count:
            self.hp.step += 1
        self._call(dL_dtau_sum, dL_dexposure if self.optimise_exposure else None, frame_status)

    def camera(self) -> Dict:
        return dict(viewmatrix=self.viewmatrix, projmatrix=self.projmatrix, projmatrix_raw=self.proj,
                    campos=self.campos, tanfovx=self.tanfovx, tanfovy=self.tanfovy)


class KeyframeWindow:
    """The mapping window's keyframes — pose, exposure and their optimiser — resident on the GPU as [V,80] pose states
    (olsr_pose_step's layout) and advanced by ONE kernel per mapping iteration (olsr_window_pose_step, one wave per view).
    It is the reference's `keyframe_optimizers` (utils/slam_backend.py:933-980) plus the update_pose calls after its step
    (:756-765): view v of the window optimises pose and exposure when v < pose_window, its exposure alone beyond, and
    nothing when its id is frozen (frame 0, which anchors the map).  MappingStep(window=...) writes every view's
    dL_dtau_sum and dL_dexposure straight into `grad_tau[v]` / `grad_exposure[v]` and calls step() once per iteration.

    A view's flags are fixed between two rebuilds: its pose and exposure groups share one step count, so a group that
    joined later would run on the others' bias corrections.  The reference builds a fresh optimiser at every new keyframe
    instead, and so does rebuild()."""

    def __init__(self, T_w2c, ids: Sequence[int], projection_matrix: torch.Tensor, tanfovx: float, tanfovy: float,
                 exposures=None, pose_window=5, frozen_ids=(0,), lr_rot=0.0015, lr_trans=0.0005, lr_exposure=0.01,
                 betas=(0.9, 0.999), eps=1e-8, converged_threshold=1e-4, device_step_count=False):
        """T_w2c: [V,4,4] (or a sequence of [4,4]) on the GPU, the window's poses in window order; ids: a stable id per view
        (the keyframe's frame index); exposures: [V,2] {a, b} per view or None (zeros); device_step_count: as in PoseState
        (every view counts its own steps in status[v][1]; needed for a gated step)."""
        if not isinstance(projection_matrix, torch.Tensor) or not projection_matrix.is_cuda:
            raise RuntimeError("KeyframeWindow: the projection matrix and the poses live on the GPU (there is no CPU path)")
        self.proj = projection_matrix.detach().to(dtype=torch.float32).contiguous()
        self.device = self.proj.device
        self.tanfovx, self.tanfovy = float(tanfovx), float(tanfovy)
        self.pose_window, self.frozen_ids = int(pose_window), tuple(frozen_ids)
        self.device_step_count = bool(device_step_count)
        self.hp = _abi.OlsrPoseParams(lr_rot=lr_rot, lr_trans=lr_trans, lr_exposure=lr_exposure, beta1=betas[0],
                                      beta2=betas[1], eps=eps, converged_threshold=converged_threshold, step=0)
        self.ids = []
        self.rebuild(ids, T_w2c, exposures)

    def __len__(self):
        return len(self.ids)

    def rebuild(self, ids: Sequence[int], T_w2c=None, exposures=None):
        """The window changed (a new keyframe): the reference's re-creation of keyframe_optimizers.  ids: the new window in
        order; T_w2c / exposures: sequences aligned with ids — an entry (or the whole argument) may be None for an id that
        was in the window before, which keeps the pose / exposure it has; a new id needs its pose (exposure: zeros).  Every
        optimiser word and count starts from zero.  Views handed out by camera() / exposure() before this call are stale."""
        ids = [int(i) for i in ids]
        V = len(ids)
        if not 1 <= V <= _abi.WINDOW_MAX_VIEWS or len(set(ids)) != V:
            raise ValueError(f"KeyframeWindow: between 1 and {_abi.WINDOW_MAX_VIEWS} distinct view ids")
        f32 = dict(dtype=torch.float32, device=self.device)
        old = {i: v for v, i in enumerate(self.ids)}
        state = torch.zeros(V, 80, **f32)
        for v, i in enumerate(ids):
            T = T_w2c[v] if T_w2c is not None else None
            e = exposures[v] if exposures is not None else None
            if T is None:
                if i not in old:
                    raise ValueError(f"KeyframeWindow: view {i} is new to the window and needs a pose")
                state[v, 0:16] = self.state[old[i], 0:16]
            else:
                state[v, 0:16] = torch.as_tensor(T).detach().to(**f32).reshape(16)
            if e is not None:
                state[v, 70:72] = torch.as_tensor(e, dtype=torch.float32).detach().to(**f32).reshape(2)
            elif i in old:
                state[v, 70:72] = self.state[old[i], 70:72]
        self.ids = ids
        self.state = state
        self.status = torch.zeros(V, 2, dtype=torch.int32, device=self.device)
        self.grad_tau = torch.zeros(V, 6, **f32)        # [rho | theta] per view, as olsr_backward leaves it
        self.grad_exposure = torch.zeros(V, 2, **f32)
        self.flags = [0 if i in self.frozen_ids else
                      (_abi.WINDOW_OPT_POSE | _abi.WINDOW_OPT_EXPOSURE if v < self.pose_window else _abi.WINDOW_OPT_EXPOSURE)
                      for v, i in enumerate(ids)]
        self._flags_c = (C.c_int32 * V)(*self.flags)
        self._zero_flags = (C.c_int32 * V)()
        self.hp.step = 0
        # (the views are made once: a mapping iteration asks for every view's camera)
        self._cameras = [dict(viewmatrix=st[16:32].view(4, 4), projmatrix=st[32:48].view(4, 4), projmatrix_raw=self.proj,
                              campos=st[48:51], tanfovx=self.tanfovx, tanfovy=self.tanfovy) for st in state]
        self._exposures = [st[70:72] for st in state]
        self._call(self._zero_flags, None)   # the matrices of the poses as they are (no flags: no step)

    def _call(self, flags, frame_status):
        check(lib().olsr_window_pose_step(C.byref(self.hp), len(self.ids), flags, self.grad_tau.data_ptr(),
                                          self.grad_exposure.data_ptr(), self.proj.data_ptr(), self.state.data_ptr(),
                                          self.status.data_ptr(),
                                          frame_status.data_ptr() if frame_status is not None else None,
                                          stream_ptr(self.device)))

    def step(self, frame_status: Optional[torch.Tensor] = None):
        """keyframe_optimizers.step() and update_pose of every view, from the gradients in grad_tau / grad_exposure.
        frame_status: device int32[V,2], per view the {R, status} of the forward its gradient came from — a view whose frame
        was not usable takes no step (needs device_step_count, as PoseState.step)."""
        if frame_status is not None:
            if not self.device_step_count:
                raise ValueError("a gated window step needs KeyframeWindow(device_step_count=True)")
            if (not frame_status.is_cuda or frame_status.dtype != torch.int32 or tuple(frame_status.shape) != (len(self.ids), 2)
                    or not frame_status.is_contiguous()):
                raise RuntimeError("KeyframeWindow.step: frame_status must be a contiguous int32 [V,2] tensor on the GPU")
        if not self.device_step_count:
            self.hp.step += 1
        self._call(self._flags_c, frame_status)

    def camera(self, v: int) -> Dict:
        """View v's camera as views of its state (the dict shape of PoseState.camera()): always the current pose."""
        return self._cameras[v]

    def exposure(self, v: int) -> torch.Tensor:
        """View v's {exposure_a, exposure_b}, a view of its state."""
        return self._exposures[v]

    def T_w2c(self, v: int) -> torch.Tensor:
        return self.state[v, 0:16].view(4, 4)


class TrackingLoop:
    """render -> tracking loss -> pose-only backward -> pose step, allocation-free and without a host sync unless the
    caller asks for the convergence flag (the reference reads it back every iteration: `converged = update_pose(...)`)."""

    def __init__(self, workspace: RasterWorkspace, gaussians: Dict[str, torch.Tensor], sh_degree: int, pose: PoseState,
                 gt_image: torch.Tensor, gt_depth: torch.Tensor, grad_mask: Optional[torch.Tensor] = None,
                 alpha=0.95, rgb_boundary_threshold=0.01, language_cotangent: str = "null", fused_loss: bool = True):
        """language_cotangent: "null" — olsr_backward gets no language cotangent (what the tracking loss means; the RGB
        instantiation of the composite backward runs); "zeros" — a zero-filled [F,H,W] cotangent through the language
        backward (what autograd materialises for the reference, kept for comparison)."""
        assert language_cotangent in ("null", "zeros")
        self.ws, self.g, self.sh_degree, self.pose = workspace, gaussians, sh_degree, pose
        # fused_loss (default): the tracking loss is evaluated in the forward composite's epilogue (olsr_forward_async_loss):
        # no loss kernel, no image round trip, the images themselves are not written.  False: olsr_forward_async +
        # olsr_tracking_loss, the two-kernel path (same cotangents bit for bit; tests/test_gpu_loss.py).
        self.fused = bool(fused_loss)
        f32 = dict(device=workspace.device, dtype=torch.float32)
        gt_image, gt_depth = gt_image.detach().to(**f32).contiguous(), gt_depth.detach().to(**f32).contiguous()
        if gt_depth.dim() == 3:
            gt_depth = gt_depth.reshape(gt_depth.shape[-2], gt_depth.shape[-1])
        if grad_mask is not None:
            grad_mask = grad_mask.detach().to(**f32).reshape(gt_depth.shape).contiguous()
        self.gt_image, self.gt_depth, self.grad_mask = gt_image, gt_depth, grad_mask
        self.alpha, self.thr = alpha, rgb_boundary_threshold
        dev = workspace.device
        self.zero_lang = (torch.zeros(workspace.F, workspace.H, workspace.W, device=dev)
                          if (language_cotangent == "zeros" and workspace.F > 0) else None)
        self.loss = None

    # (Round 3 offered TrackingLoop.capture(): the iteration recorded into a HIP graph.  It is a fixed launch sequence on
    #  device-resident state — PoseState(device_step_count=True) — and replays bit-identically, which tests/test_gpu_pose.py
    #  still proves with its own capture.  As a product entry it is gone: measured in rounds 3 and 4 the replay is SLOWER than
    #  issuing the launches (0.607 vs 0.587 ms, then 0.567 vs 0.549 ms: the iteration is bound by its dependent kernels, not by
    #  the host), and the capture's extra streams pushed a process past its four hardware queues, which slowed every later
    #  four-lane run by 12 %.  VERDICT round 3, next #9.)

    def iteration(self, read_convergence=False, write_images=False) -> bool:
        """write_images: also write this iteration's images into ws.out (colour, depth, opacity and — on a language workspace —
        the language map).  The fused iteration skips them by default (nothing reads them between two tracking iterations, and
        on a language workspace the F = 0 composite runs), so ws.out keeps STALE data; the reference's front end reads the LAST
        tracking iteration's render_pkg["depth"] / ["opacity"] / ["render"] for add_new_keyframe, the GUI and the evaluation
        (utils/slam_frontend.py:664-665): pass write_images=True on the final (or converged) iteration, or call render_final()."""
        ws = self.ws
        ws.set_scene(sh_degree=self.sh_degree, **self.pose.camera(), **self.g)
        if self.fused:
            lo = ws.forward_loss(self.gt_image, self.gt_depth, None, self.pose.exposure, self.grad_mask, tracking=True,
                                 alpha=self.alpha, rgb_boundary_threshold=self.thr, skip_images=not write_images)
        else:
            out = ws.forward()
            lo = losses.tracking_loss(out["color"], out["depth"], out["opacity"], self.gt_image, self.gt_depth,
                                      self.grad_mask, self.pose.exposure, alpha=self.alpha,
                                      rgb_boundary_threshold=self.thr)
        self.loss = lo["loss"]
        g = ws.backward(lo["dL_dimage"], self.zero_lang, lo["dL_ddepth"], pose_only=True)
        # Per-tile depth cut-offs (RasterWorkspace(depth_cut=True), include/olsr.h): every iteration renders with the cut-offs
        # the previous one left.  A frame whose cut-offs hid something is flagged on the device; its backward writes zeros and
        # the gated pose step does nothing, so the iteration is a no-op and the next one renders the offending tiles uncut:
        # the k-th COUNTED step sees the pose the k-th step of the loop without cut-offs sees; `steps_done()` says how many
        # iterations counted, and run(steps) iterates until that many did (a fixed budget of iterations would otherwise take
        # fewer optimiser steps than the reference's tracking_itr_num - ADVICE round 4).
        self.pose.step(g["dL_dtau_sum"], lo["dL_dexposure"],
                       frame_status=ws.num_rendered if ws.depth_cut is not None else None)
        if read_convergence:
            return bool(int(self.pose.status[0].item()))  # one 4-byte read-back, like the reference
        return False

    def run(self, steps: int, check_every: int = 16, max_iterations: Optional[int] = None, write_final_images=False) -> int:
        """Iterate until `steps` optimiser steps have been taken (the reference's tracking_itr_num), the way its loop does
        with a fixed budget — but counting only iterations whose frame was usable: with per-tile depth cut-offs an iteration
        whose frame missed is a device-side no-op.  The count lives on the device; it is read back every `check_every`
        iterations (one 4-byte copy each), so the loop overshoots by at most nothing: it first issues the iterations that are
        certainly needed (steps - done), then looks again.  Without cut-offs every iteration counts and nothing is read back.
        Returns the number of iterations issued."""
        issued = 0
        limit = max_iterations if max_iterations is not None else 4 * steps + 16
        if self.ws.depth_cut is None:
            for k in range(steps):
                self.iteration(write_images=write_final_images and k == steps - 1)
            return steps
        done = self.steps_done()
        target = done + steps
        while done < target and issued < limit:
            for _ in range(min(target - done, check_every, limit - issued)):
                self.iteration()
                issued += 1
            done = self.steps_done()
        if write_final_images:
            self.render_final()
        return issued

    def render_final(self) -> Dict[str, torch.Tensor]:
        """The images of the CURRENT pose (after the last pose step): one plain forward into ws.out, for add_new_keyframe / GUI /
        evaluation.  No loss, no pose step.  Which pose: the reference's front end keeps the render_pkg of its LAST ITERATION,
        i.e. of the pose BEFORE the last step (utils/slam_frontend.py:216-243) — iteration(write_images=True) on the final
        iteration, and run(write_final_images=True) without depth cut-offs, leave exactly those; render_final(), and
        run(write_final_images=True) WITH depth cut-offs (whose iterations write no images), leave the images one step later,
        of the pose the loop ends with.  The two differ by one optimiser step of a converged loop."""
        ws = self.ws
        # (never through the depth cut-offs — ADVICE round 5: a CUT_MISS frame would leave depth / opacity / colour with missing
        #  contributions, and nothing downstream of these images looks at the forward's status.  The cut-off array itself is
        #  left as the last iteration left it.)
        keep_cut, ws._depth_cut_buf = ws._depth_cut_buf, None
        try:
            ws.set_scene(sh_degree=self.sh_degree, **self.pose.camera(), **self.g)
            return ws.forward()
        finally:
            ws._depth_cut_buf = keep_cut

    def steps_done(self) -> int:
        """Optimiser steps taken since PoseState.reset (device count; with depth cut-offs an iteration whose frame missed
        does not count)."""
        return int(self.pose.status[1].item())


def _follow_map(step) -> bool:
    """Shared by the loops that run on a GaussianMap (`step.map`, `step.lanes`, `step.params`, `step._map_edits`): take the
    map's current parameter views, tell it that this iteration's backward gives every parameter a gradient, and after a
    topology edit resize the lanes to its P.  Returns True when there was such an edit."""
    m = step.map
    step.params = m.params
    m.new_gradients()
    if m.edits == step._map_edits:
        return False
    step._map_edits = m.edits
    if step.lanes.P != m.P:
        step.lanes.resize(m.P)
    return True


class MappingStep:
    """One mapping iteration over `cameras` (all views against the same Gaussians), `lanes` views in flight, gradients
    written / added straight into the flat bucket by the backward kernel, one fused Adam step on the raw parameters."""

    def __init__(self, lanes: FrameLanes, params: Dict[str, torch.Tensor], bg: torch.Tensor, sh_degree: int,
                 cameras: Sequence[Dict], targets: Sequence, lrs: Dict[str, float], exposure=None,
                 activations=_abi.ACT_ALL, fused_loss="auto", view_ids: Optional[Sequence] = None, carry_order: Optional[bool] = None,
                 gaussian_map=None, edit_hook: Optional[Callable] = None, record_visibility: bool = False,
                 window: Optional[KeyframeWindow] = None, isotropic_weight: Optional[float] = None):
        """targets[v] = (gt_image [3,H,W], gt_depth [H,W], gt_language [F,h,w] or None).
        fused_loss: True — the mapping loss is evaluated in the forward composite's epilogue (olsr_forward_async_loss); False —
        olsr_forward_async + olsr_mapping_loss (two kernels; the same cotangents bit for bit, the loss value to summation order);
        "auto" (default, round 5) — MEASURED: iterations 3-6 of this object alternate the two forms between HIP events, the
        faster one is kept from then on (`self.fused`, `self.calibration`).  Which one wins depends on the workload: on the
        i.i.d. volume of SURVEY 8(d) four views in flight keep the vector ALU saturated and the separate, HBM-bound loss kernel
        hides beside other lanes' composites (two-kernel 2 % faster); on a surface map the frame is latency-bound and the
        fused form saves a launch and an image round trip per view (5 % faster).
        view_ids: a stable id per camera (default: its position) keying the per-view tile-order hints, so that a sliding
        keyframe window (cameras reassigned, grown or reordered between iterations) keeps every view's own order.
        carry_order (round 6): every view also keeps its DEPTH order of the previous iteration (include/olsr.h "Carried depth
        order"; 4 P bytes per view): an Adam step moves the Gaussians by a fraction of a millimetre, so the forward repairs that
        order in two launches instead of sorting from scratch in five dependent ones, and falls back to the sort on the device
        when it cannot prove the result — parameters are bit-identical either way (tests/test_gpu_order_carry.py).
        None (default) = on with ONE lane only: measured (scripts/probe/mapping_time.py, 12 views, 500 k Gaussians) it takes
        2.5 % off the iteration on the room map and 1.8 % on the volume with one view in flight (4.77 -> 4.65 ms, 8.62 -> 8.46 ms),
        nothing with two, and costs 0.5 % with four — other lanes' composites already hide the sort's dependent launches, and
        the repair's own work is then extra.
        gaussian_map (a gaussian_map.GaussianMap; `params` is then ignored): the map owns the parameters, the Adam state and
        the densification statistics, and may change P between iterations.  Each iteration then adds the step's statistics
        to the map (the reference's per-view add_densification_stats and max_radii2D update) and, before the Adam step, calls
        edit_hook(step, total_bucket) — the place of the reference's densify_and_prune / reset_opacity
        (utils/slam_backend.py:418-445, 716-752).  Whatever the hook edits, the map records which parameter groups it
        replaced; the step then skips them as the reference's optimizer.step() does (all groups after a topology edit, the
        opacity group after a reset).  The hook may return "all" or a collection of group names to skip besides.  The next
        iteration follows the map's new P (FrameLanes.resize; carried depth orders start again, tile-order hints stay).
        record_visibility: keep each view's radii > 0 and n_touched > 0 of the last iteration (self.visibility[view id],
        self.touched[view id]): the visibility filters of reset_opacity_nonvisible and the co-visibility count.
        window (a KeyframeWindow): the bundle adjustment of the reference's map().  The window's views come FIRST in
        `targets` / `view_ids` (len(window) of them, in window order) and are rendered from the window's own cameras and
        exposures; `cameras` holds only the remaining (rehearsal) views, which use the shared `exposure` and get no update,
        as in the reference.  Each window view's dL_dtau_sum and dL_dexposure are written by the kernels straight into its
        slot of the window, and after the lanes have joined ONE window step runs on the caller's stream, beside the Adam
        step (keyframe_optimizers.step() + update_pose, utils/slam_backend.py:756-765).
        isotropic_weight: the reference's `loss_mapping += 10 * |scaling - scaling.mean(dim=1)|.mean()` (:664-667) with that
        weight (the reference's: 10); its gradient is formed inside the Adam step (FusedAdam.step(isotropic=...)), its value
        is not part of `last_loss` (losses.isotropic_loss gives it).  None: no regulariser.
        With both left at None every path is what it was without them."""
        self.window = window
        self.isotropic_weight = None if isotropic_weight is None else float(isotropic_weight)
        self.map, self.edit_hook, self.record_visibility = gaussian_map, edit_hook, bool(record_visibility)
        self.visibility: Dict = {}
        self.touched: Dict = {}
        if gaussian_map is not None:
            params = gaussian_map.params
            self._map_edits = gaussian_map.edits
        self.lanes, self.params, self.bg, self.sh_degree = lanes, params, bg, sh_degree
        self.cameras, self.lrs, self.exposure, self.act = cameras, lrs, exposure, activations
        self.view_ids = view_ids
        self.auto = fused_loss == "auto"
        self.fused = True if self.auto else bool(fused_loss)
        self.calibration = None   # {"fused_ms": [...], "two_kernel_ms": [...], "chosen": ...} once "auto" has decided
        self._cal = {"n": 0, "pending": [], True: [], False: []}
        self.targets = targets
        ws0 = lanes.lanes[0][0]
        if gaussian_map is not None and ws0.P != gaussian_map.P:
            lanes.resize(gaussian_map.P)
        self.adam = gaussian_map.adam if gaussian_map is not None else FusedAdam(ws0.P, GradLayout(ws0.M, ws0.F), ws0.device)
        self.last_loss = None
        # profile = True: iteration() brackets its caller-side steps (the stand-alone loss kernel, the sum of the lane
        # buckets, the Adam step) with HIP events and leaves (name, ms) pairs in self.stage_ms — for bench.py's breakdown;
        # an event is a barrier packet on its stream, so timed runs keep it off
        self.profile = False
        self.stage_ms = []
        # Launch-order hint of the forward composite, one PER VIEW: a mapping call iterates over the same window of keyframes
        # (utils/slam_backend.py:510-670), so view v's heaviest-first tile order of the previous iteration is the right hint
        # for it — the lane's own previous frame was another view, and a stale order costs the forward composite 25-35 %
        # (measured, scripts/probe/arc_views.py: 0.17 -> 0.23 ms at config 3; the order cannot be predicted from the list
        # lengths, which correlate with the measured work at -0.4 .. 0.8).
        # (keyed by a stable view id and created lazily — ADVICE round 4: a list sized at construction broke when the window grew)
        self.view_hints: Dict = {}
        self._hint_proto = ws0.tile_order.clone()
        self.carry_order = (len(lanes) == 1) if carry_order is None else bool(carry_order)
        self.view_orders: Dict = {}   # view id -> int32[P], the view's depth order of its last iteration (zeros: none yet)

    @property
    def targets(self):
        return self._targets

    @targets.setter
    def targets(self, targets):
        """Targets are converted ONCE to contiguous float32 on the device (the reference keeps gt_lang_feat on the CPU and
        moves it every iteration, utils/slam_backend.py:576)."""
        if targets is None:
            self._targets = None
            return
        dev = self.lanes.device
        cv = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        self._targets = [(cv(a), cv(b.reshape(b.shape[-2], b.shape[-1])), cv(c)) for a, b, c in targets]

    def render(self, ws, cam):
        ws.set_scene(bg=self.bg, sh_degree=self.sh_degree, activations=self.act, **cam, **self.params)
        return ws.forward()

    def _calibrate(self, main):
        """fused_loss="auto": iterations 3-6 alternate fused / two-kernel; each is bracketed by two events on the caller's
        stream (recorded without a synchronisation); once the events of all four have completed the faster form stays."""
        c = self._cal
        done = [p for p in c["pending"] if p[2].query()]
        for p in done:
            c[p[0]].append(p[1].elapsed_time(p[2]))
            c["pending"].remove(p)
        if len(c[True]) >= 2 and len(c[False]) >= 2 and self.calibration is None:
            f, t = min(c[True]), min(c[False])
            self.fused = f <= t
            self.calibration = {"fused_ms": [round(x, 4) for x in c[True]], "two_kernel_ms": [round(x, 4) for x in c[False]],
                                "chosen": "fused" if self.fused else "two_kernel"}
            self.auto = False
            return None
        c["n"] += 1
        if 3 <= c["n"] <= 6 or (c["n"] > 6 and not c["pending"] and self.calibration is None):
            self.fused = (c["n"] % 2 == 1)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(main)
            return ev
        return None

    def _follow_map(self):
        """A map edit since the last iteration: take the map's parameter views, resize the lanes to its P, drop the carried
        depth orders (they index the old rows; the tile-order hints are per tile and stay)."""
        if _follow_map(self):
            self.view_orders = {}
            self.visibility, self.touched = {}, {}

    def iteration(self, stats: bool = True):
        """stats=False (with a map): the statistics of this iteration are not added — the reference's co-visibility prune
        iteration returns before add_densification_stats (utils/slam_backend.py:683-716)."""
        if self.map is not None:
            self._follow_map()
        lanes = self.lanes
        dev = lanes.device
        used = []
        main = torch.cuda.current_stream(dev)
        marks = []
        cal_ev = self._calibrate(main) if self.auto else None
        cal_form = self.fused

        def mark(name, stream):
            if self.profile:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(stream)
                marks.append((name, ev))
        for _, _, st in lanes.lanes:  # the parameters (and, the first time, the targets) were written on the caller's stream
            if st != main:
                st.wait_stream(main)
        win = self.window
        nw = len(win) if win is not None else 0
        for v in range(nw + len(self.cameras)):
            cam = win.camera(v) if v < nw else self.cameras[v - nw]
            exposure = win.exposure(v) if v < nw else self.exposure
            dexp_out = win.grad_exposure[v] if v < nw else None
            ws, bucket, stream = lanes.next_lane()
            first = bucket not in used
            if first:
                used.append(bucket)
            vid = self.view_ids[v] if self.view_ids is not None else v
            if vid not in self.view_hints or (self.carry_order and vid not in self.view_orders):
                # (created on the caller's stream, which the lanes are ordered behind)
                if vid not in self.view_hints:
                    self.view_hints[vid] = self._hint_proto.clone()
                if self.carry_order:
                    self.view_orders[vid] = torch.zeros(ws.P, dtype=torch.int32, device=dev)
                stream.wait_stream(main)
            with torch.cuda.stream(stream):
                ws.tile_order = self.view_hints[vid]   # in: this view's order of the last iteration; out: this iteration's
                ws.depth_order_carry = self.view_orders[vid] if self.carry_order else None
                if self.fused:
                    ws.set_scene(bg=self.bg, sh_degree=self.sh_degree, activations=self.act, **cam, **self.params)
                    lo = ws.forward_loss(*self.targets[v], exposure, skip_images=True, dL_dexposure_out=dexp_out)
                else:
                    out = self.render(ws, cam)
                    mark("loss:begin", stream)
                    lo = losses.mapping_loss(out["color"], out["depth"], out["language"] if ws.F > 0 else None,
                                             *self.targets[v], exposure, dL_dexposure_out=dexp_out)
                    mark("loss:end", stream)
                    if ws.F > 0 and self.targets[v][2] is None:
                        lo["dL_dlanguage"] = None
                if self.record_visibility:
                    self.visibility[vid] = ws.out["radii"] > 0
                    self.touched[vid] = ws.out["n_touched"] > 0
                ws.backward(lo["dL_dimage"], lo["dL_dlanguage"], lo["dL_ddepth"], bucket=bucket, first=first,
                            bucket_only=True, tau_sum_out=win.grad_tau[v] if v < nw else None)
                self.last_loss = lo["loss"]
        for _, _, st in lanes.lanes:
            main.wait_stream(st)
        total = used[0]
        from .frame_shard import GradientBucket
        multi = GradientBucket._multi()
        mark("lane_sum:begin", main)
        for i, b in enumerate(used[1:], 1):
            if multi:   # an exchange follows: it needs the total in one place (only the rows b's row mask flags move)
                total.add_bucket(b)
            elif i < 8:  # one process: only the small densification statistics are summed, Adam adds the gradient rows itself
                total.densify.add_(b.densify)
                torch.maximum(total.max_radii, b.max_radii, out=total.max_radii)
            # (lanes beyond the eighth are folded into the first bucket below by add_bucket, which sums their statistics
            #  and radii as well — adding them here too counted them twice: ADVICE round 5, medium)
        mark("lane_sum:end", main)
        total.all_reduce()
        mark("adam:begin", main)
        if not multi and len(used) > 8:   # (olsr_adam_step_masked sums at most eight buckets: fold the rest into the first)
            for b in used[8:]:
                used[0].add_bucket(b)
            used = used[:8]
        if self.map is None:
            self.adam.step(total if multi else used, self.params, self.lrs, isotropic=self.isotropic_weight,
                           activations=self.act)
        else:
            if stats:
                self.map.add_densification_stats(total)
            skip = self.edit_hook(self, total) if self.edit_hook is not None else None
            self.map.step(total if multi else used, self.lrs, skip=skip or (), isotropic=self.isotropic_weight,
                          activations=self.act)
            self.params = self.map.params
        mark("adam:end", main)
        if win is not None:   # (the lanes have joined: every view's gradient slots are written)
            win.step()
        if cal_ev is not None:
            end = torch.cuda.Event(enable_timing=True)
            end.record(main)
            self._cal["pending"].append((cal_form, cal_ev, end))
        for _, _, st in lanes.lanes:
            st.wait_stream(main)
        # (single process: total.flat holds lane 0's rows ONLY — the sum over the lanes exists inside the Adam kernel, not in any
        #  bucket; total.densify / total.max_radii are the step's totals.  A caller that wants the summed gradient rows calls
        #  summed_gradients(), which adds the lane buckets into a copy.)
        self._used = used
        if self.profile:
            torch.cuda.synchronize(dev)
            self.stage_ms = []
            open_ = {}
            for name, ev in marks:
                stage, edge = name.split(":")
                if edge == "begin":
                    open_[stage] = ev
                else:
                    self.stage_ms.append((stage, open_.pop(stage).elapsed_time(ev)))
        return total

    def summed_gradients(self) -> torch.Tensor:
        """[P, width] gradient rows of the last iteration summed over the lanes (a fresh tensor): in a single process the
        iteration's return value holds lane 0's rows only."""
        from .frame_shard import GradientBucket
        out = self._used[0].flat.clone()
        if not GradientBucket._multi():   # (with an exchange ahead the lanes were already summed into the first bucket)
            for b in self._used[1:]:
                out.add_(b.flat)
        return out


def position_lr(step: int, lr_init: float, lr_final: float, max_steps: int) -> float:
    """The reference's position learning-rate schedule without delay (gaussian_splatting/utils/general_utils.py:79-94):
    log-linear from lr_init at step 0 to lr_final at max_steps, constant after; 0 for a negative step or a disabled group."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)


class RefinementStep:
    """The colour-refinement loop on the fused path: per iteration ONE view -> forward -> olsr_refinement_loss -> backward
    into the bucket -> max_radii2D of that view -> one Adam step on every group -> the xyz rate of the next step.

    Two details of the reference are kept.  Its render() goes through the language rasterizer when the map has language
    features (gaussian_renderer/__init__.py:39-48) while the loss reads the colour image only: autograd hands the
    rasterizer a zero language cotangent and optimizer.step() steps the language group with a zero gradient (its moments
    decay, the leftover momentum still moves it) - here the backward gets a NULL language cotangent, writes zeros into the
    bucket's language columns, and the group is stepped like the others.  And only max_radii2D is updated
    (utils/slam_backend.py:809-812): the densification statistics are not.
    Iterations depend on each other, so one lane (the first of `lanes`) is used; `last_loss` stays on the device."""

    def __init__(self, lanes: FrameLanes, params: Optional[Dict[str, torch.Tensor]], bg: torch.Tensor, sh_degree: int,
                 cameras: Sequence[Dict], gt_images: Sequence[torch.Tensor], lrs: Dict[str, float], lambda_dssim: float = 0.2,
                 position_schedule=None, activations=_abi.ACT_ALL, view_ids: Optional[Sequence] = None, gaussian_map=None,
                 adam: Optional[FusedAdam] = None):
        """gt_images[v]: [3,H,W], converted once to contiguous float32 on the device.
        position_schedule = (lr_init, lr_final, max_steps): step i (from 0) runs with xyz rate position_lr(i, ...), as the
        reference's update_learning_rate(iteration) after every step leaves it (its first step runs with the group's
        configured rate, which is lr_init); None keeps lrs["xyz"].
        gaussian_map (`params` is then ignored): the map owns the parameters, the Adam state and max_radii2D; otherwise
        `params` + `adam` (a FusedAdam; a fresh one when None), and max_radii2D is kept in self.max_radii.
        view_ids: a stable id per camera keying the per-view tile-order hints (default: its position)."""
        self.map = gaussian_map
        if gaussian_map is not None:
            params = gaussian_map.params
            self._map_edits = gaussian_map.edits
        self.lanes, self.params, self.bg, self.sh_degree = lanes, params, bg, sh_degree
        self.cameras, self.lrs, self.act, self.view_ids = cameras, dict(lrs), activations, view_ids
        self.lambda_dssim = float(lambda_dssim)
        ws0 = lanes.lanes[0][0]
        dev = lanes.device
        if gaussian_map is not None and ws0.P != gaussian_map.P:
            lanes.resize(gaussian_map.P)
        if len(gt_images) != len(cameras):
            raise ValueError("RefinementStep: one ground-truth image per camera")
        self.gt_images = [g.detach().to(device=dev, dtype=torch.float32).contiguous() for g in gt_images]
        if gaussian_map is not None:
            self.adam = gaussian_map.adam
            self.max_radii = None
        else:
            self.adam = adam if adam is not None else FusedAdam(ws0.P, GradLayout(ws0.M, ws0.F), dev)
            self.max_radii = torch.zeros(ws0.P, dtype=torch.int32, device=dev)
        self.schedule = tuple(position_schedule) if position_schedule is not None else None
        self.steps = 0
        self.xyz_lr = position_lr(0, *self.schedule) if self.schedule is not None else self.lrs["xyz"]
        self.last_xyz_lr = None   # the rate the last iteration's step ran with
        self.last_view = None
        self.last_loss = None
        self.view_hints: Dict = {}
        self._hint_proto = ws0.tile_order.clone()
        self._loss_buffers: Dict = {}

    def loss(self, image, gt_image):
        """dict(loss[4], dL_dimage) of one view (olsr_refinement_loss; the buffers are reused between iterations)."""
        return losses.refinement_loss(image, gt_image, lambda_dssim=self.lambda_dssim, buffers=self._loss_buffers)

    def iteration(self, view: Optional[int] = None):
        """view: index into `cameras`; None draws one like the reference does (random.randint over the keyframes)."""
        if self.map is not None:
            _follow_map(self)
        v = random.randint(0, len(self.cameras) - 1) if view is None else int(view)
        ws, bucket, _ = self.lanes.lanes[0]
        vid = self.view_ids[v] if self.view_ids is not None else v
        if vid not in self.view_hints:
            self.view_hints[vid] = self._hint_proto.clone()
        ws.tile_order = self.view_hints[vid]   # in: this view's order of its last iteration; out: this iteration's
        ws.depth_order_carry = None            # (a view comes back after many Adam steps: its old depth order proves nothing)
        ws.set_scene(bg=self.bg, sh_degree=self.sh_degree, activations=self.act, **self.cameras[v], **self.params)
        out = ws.forward()
        lo = self.loss(out["color"], self.gt_images[v])
        ws.backward(lo["dL_dimage"], None, None, bucket=bucket, first=True, bucket_only=True)
        self.last_loss, self.last_view = lo["loss"], v
        lrs = dict(self.lrs, xyz=self.xyz_lr)
        max_radii = self.map.max_radii if self.map is not None else self.max_radii
        torch.maximum(max_radii, bucket.max_radii, out=max_radii)
        if self.map is not None:
            self.map.step([bucket], lrs)   # (honours the groups an edit since the last backward replaced: none here)
        else:
            self.adam.step([bucket], self.params, lrs)
        self.last_xyz_lr = self.xyz_lr
        self.steps += 1
        if self.schedule is not None:
            self.xyz_lr = position_lr(self.steps, *self.schedule)
        return bucket

    def run(self, n: int, views: Optional[Sequence[int]] = None):
        """n iterations; views: the view of each (len n), else random ones."""
        for i in range(n):
            self.iteration(None if views is None else views[i])
        return self.last_loss


class OnlineLanguageTargets:
    """The language targets of the mapping loop, produced the way the reference's map() produces them: the online autoencoder
    (lang_codec.OnlineLanguageCodec) takes one training step on a new keyframe's 32-channel features and the codes of that
    step's forward pass become the keyframe's [15,h,w] target (utils/slam_backend.py:562-576); the two random rehearsal views of
    every mapping iteration train it once more each and keep the targets they have (:640-648).  Features and targets stay on
    the device (the reference keeps gt_lang_feat on the CPU and uploads it every iteration)."""

    def __init__(self, codec, lr: float = 1e-4, hw=(192, 192)):
        """lr: 1e-4 in map(), 1e-3 during initialize_map."""
        self.codec, self.lr, self.hw = codec, float(lr), (int(hw[0]), int(hw[1]))
        self.features: Dict = {}
        self.targets: Dict = {}
        self.steps = 0
        self.last_loss = None   # loss[4] of the last step, a copy (the codec's own loss buffer is overwritten by every step)

    def add_keyframe(self, view_id, features32: torch.Tensor) -> torch.Tensor:
        """features32 [h*w,32] (or [h,w,32]) float32 on the codec's device: one train step, the codes of its forward pass are
        stored as the view's [15,h,w] target.  The features are copied: the caller may reuse its buffer.  -> that target."""
        h, w = self.hw
        if isinstance(features32, torch.Tensor) and features32.dim() == 3:
            features32 = features32.reshape(-1, features32.shape[-1])
        if not isinstance(features32, torch.Tensor) or features32.dim() != 2 or features32.shape[0] != h * w:
            raise RuntimeError(f"add_keyframe: features must be [{h * w},32] for hw = {self.hw}")
        loss, codes = self.codec.train_step(features32, self.lr, codes="pre", layout="channels")
        self.features[view_id] = features32.detach().clone()
        self.targets[view_id] = codes.clone().view(codes.shape[0], h, w)
        self.steps += 1
        self.last_loss = loss.clone()
        return self.targets[view_id]

    def add_keyframe_hr(self, view_id, hr_features: torch.Tensor, encoder) -> torch.Tensor:
        """hr_features [1,768,h,w] (or [768,h,w], or [h*w,768] rows) float32 on the codec's device, encoder a
        lang_encoder.LanguageEncoder: the general encoder writes the view's [h*w,32] rows straight into the buffer kept for
        rehearsal (utils/slam_backend.py:556-559), then the train step of add_keyframe on them.  -> the [15,h,w] target."""
        h, w = self.hw
        feats = torch.empty(h * w, _abi.LANG_AE_IN, dtype=torch.float32, device=self.codec.device)
        try:
            encoder.encode(hr_features, out=feats)
        except OlsrError:
            raise
        except RuntimeError as e:
            raise RuntimeError(f"add_keyframe_hr: features must encode to [{h * w},32] for hw = {self.hw}: {e}") from e
        loss, codes = self.codec.train_step(feats, self.lr, codes="pre", layout="channels")
        self.features[view_id] = feats
        self.targets[view_id] = codes.clone().view(codes.shape[0], h, w)
        self.steps += 1
        self.last_loss = loss.clone()
        return self.targets[view_id]

    def add_keyframe_backbone(self, view_id, fv: torch.Tensor, f3: torch.Tensor, f2: torch.Tensor, hr_net, encoder) -> torch.Tensor:
        """fv [1,768,h/8,w/8], f3 [1,384,.,.], f2 [1,192,.,.]: the backbone's clip_vis_dense, res3 and res2 on the codec's
        device; hr_net an hr_net.HighResLanguageNet, encoder a lang_encoder.LanguageEncoder.  The high-resolution net turns
        them into the [1,768,h,w] map (a buffer of hr_net's, overwritten by its next call), then add_keyframe_hr on that map:
        utils/slam_backend.py:547-576 from the backbone's three maps to the stored target.  -> the [15,h,w] target."""
        return self.add_keyframe_hr(view_id, hr_net.forward(fv, f3, f2), encoder)

    def rehearse(self, view_ids: Sequence) -> None:
        """One train step on the stored features of each id; their targets stay as they are."""
        for v in view_ids:
            if v not in self.features:
                raise KeyError(f"rehearse: view {v!r} was never added")
        loss = None
        for v in view_ids:
            loss, _ = self.codec.train_step(self.features[v], self.lr, codes=None)
            self.steps += 1
        if loss is not None:
            self.last_loss = loss.clone()

    def targets_for(self, view_ids: Sequence):
        """The third slot of MappingStep.targets for these views, in order."""
        return [self.targets[v] for v in view_ids]
