"""A pure-Python model of the schedule an online SLAM session runs, written from the reference's loops
(utils/slam_backend.py:348-449 initialize_map, :499-767 map, :918-990 the keyframe message; utils/slam_frontend.py:585-676):
which mapping iterations run with how many views, at which iteration counts the map is densified or its opacities reset,
and after which keyframes the co-visibility prune runs.  It is fed a run's own keyframe decisions and window contents and
returns the trace `OnlineSlam.events` must equal (tests/test_gpu_online_slam.py).  No torch, no GPU.

What it cannot know — the sizes a prune leaves — is dropped from both sides by `normalise`."""

SMALL_CONFIG = {
    "Dataset": {"type": "replica", "pcd_downsample": 16, "pcd_downsample_init": 8, "point_size": 0.05, "adaptive_pointsize": True},
    "Training": {"init_itr_num": 60, "init_gaussian_update": 20, "init_gaussian_reset": 100000, "init_gaussian_th": 0.005,
                 "init_gaussian_extent": 30, "tracking_itr_num": 20, "mapping_itr_num": 10, "gaussian_update_every": 10,
                 "gaussian_update_offset": 5, "gaussian_th": 0.3, "gaussian_extent": 1.0, "gaussian_reset": 7,
                 "size_threshold": 20, "kf_interval": 2, "window_size": 4, "pose_window": 2, "edge_threshold": 1.1,
                 "rgb_boundary_threshold": 0.01, "kf_translation": 0.01, "kf_min_translation": 0.005, "kf_overlap": 0.99,
                 "prune_mode": "slam", "use_gt_pose": False, "single_thread": True, "alpha": 0.95, "seed": 11,
                 "lr": {"cam_rot_delta": 0.003, "cam_trans_delta": 0.001}},
    "opt_params": {"position_lr_init": 0.00016, "position_lr_final": 0.0000016, "position_lr_max_steps": 30000,
                   "feature_lr": 0.0025, "language_lr": 0.0025, "opacity_lr": 0.05, "scaling_lr": 0.001, "rotation_lr": 0.001,
                   "percent_dense": 0.01, "lambda_dssim": 0.2, "densify_from_iter": 100000, "densify_grad_threshold": 0.0002},
    "language": {"language_train": True, "single_stage_ae": True, "lang_code_size": 15, "labels_from_file": True},
}


def normalise(events):
    """A session's events as the model can predict them: ("prune", P_before, P_after) -> ("prune",)."""
    return [("prune",) if e[0] == "prune" else tuple(e) for e in events]


def schedule(config, frames, language):
    """frames: per tracked frame, in order, dict(idx, iterations, is_keyframe, window) — `window` the window after the frame
    (newest first), `iterations` the tracking iterations it took; frames[0] is the frame the map was initialised from.
    language: the session supervises language (a ("language", kf) event the first time a keyframe is mapped).
    -> the list of events."""
    T, O = config["Training"], config["opt_params"]
    ev, count = [], 0
    first = frames[0]["idx"]
    ev.append(("init", first))
    for k in range(T["init_itr_num"]):                       # initialize_map
        count += 1
        ev.append(("map", count, 1))
        if k % T["init_gaussian_update"] == 0:
            ev.append(("densify", count))
        if count == T["init_gaussian_reset"] or count == O["densify_from_iter"]:
            ev.append(("reset_opacity", count))
    keyframes, window, with_target = [first], [first], set()
    for f in frames[1:]:
        ev.append(("track", f["idx"], f["iterations"]))
        assert 0 <= f["iterations"] <= T["tracking_itr_num"]
        if not f["is_keyframe"]:
            assert list(f["window"]) == window, "a frame that is no keyframe leaves the window alone"
            continue
        # single-thread rule: create_kf = check_time and create_kf
        assert f["idx"] - window[0] >= T["kf_interval"], "a keyframe before kf_interval frames have passed"
        new = list(f["window"])
        assert new[0] == f["idx"] and set(new[1:]) <= set(window) and len(new) <= T["window_size"]
        ev.append(("keyframe", f["idx"], tuple(new)))
        ev.extend(("removed", k) for k in window if k not in new)
        keyframes.append(f["idx"])
        window = new
        if language:
            for k in window:                                 # gt_lang_feat is made the first time a view is mapped
                if k not in with_target:
                    with_target.add(k)
                    ev.append(("language", k))
        outside = sum(1 for k in keyframes if k not in window)
        for _ in range(T["mapping_itr_num"]):                # map(current_window, iters=mapping_itr_num, lang_run=True)
            count += 1
            ev.append(("map", count, len(window) + min(2, outside)))
            if count % T["gaussian_update_every"] == T["gaussian_update_offset"]:
                ev.append(("densify", count))
            elif count % T["gaussian_reset"] == 0:
                ev.append(("reset_opacity", count))
        count += 1                                           # map(current_window, prune=True)
        if len(window) == T["window_size"]:
            ev.append(("prune",))
    return ev
