"""The map's PLY record on the device (olsr_map_ply_pack / olsr_map_ply_unpack, csrc/k_map_io.hip), the files
(GaussianMap.save_ply / load_ply / save_state / load_state) and the session's save_gaussians, against the numpy restatement of
the reference's record (tests/map_io_ref.py).

Both kernels only move words, so every comparison is exact and made on int32 views; the values are random bit patterns with
NaNs of several payloads (quiet and signalling), +-0, +-inf and denormals planted.  Shapes (P, M, F):
    (1, 1, 15)      one row                                   (255, 1, 15)   one row short of four 64-row blocks, width 32
    (256, 1, 0)     exactly four blocks; width 17: no row of the record array is 16-byte aligned but every fourth
    (257, 4, 3)     one row into a fifth block; the f_rest transposition at M = 4; width 29
    (1000, 16, 15)  the transposition at M = 16; width 77       (513, 1, 32)   the widest language record; width 46
The map's capacity exceeds P and the rows from P on hold a sentinel that must never appear in an output."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import map_io_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 15), (255, 1, 15), (256, 1, 0), (257, 4, 3), (1000, 16, 15), (513, 1, 32)]
PARAMS = ("means3D", "shs", "opacities", "scales", "rotations", "language")
LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)
SPARE = 70    # rows of capacity beyond P: more than one block of rows

_CASES = {}


def case(P, M, F):
    """The shape's inputs (numpy, random bits) and the restated record, made once."""
    if (P, M, F) not in _CASES:
        a = R.random_map(P, M, F, seed=1000 * M + 10 * F + P)
        _CASES[(P, M, F)] = (a, R.record(a["means3D"], a["shs"], a["opacities"], a["scales"], a["rotations"], a["language"]))
    return _CASES[(P, M, F)]


def sentinel_fill(t):
    if t.numel():
        t.view(-1).view(torch.int32).fill_(R.SENTINEL)


def buffers(m):
    return m._bufs[m._front]


def make_map(a, M, F, capacity):
    """A GaussianMap holding the arrays `a`; every row from P on, of every buffer, holds the sentinel."""
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    t = {k: torch.from_numpy(v).to(DEV) for k, v in a.items()}
    m = GaussianMap(t["means3D"], t["shs"], t["opacities"], t["scales"], t["rotations"], t["language"] if F else None, LRS,
                    capacity=capacity, device=DEV)
    assert (m.M, m.F, m.capacity) == (M, F, capacity)
    for k, v in buffers(m).items():
        if k != "cap":
            sentinel_fill(v[m.P:])
    return m


def bits(t):
    return R.bits(t.detach().cpu().numpy())


def assert_params(m, a, what):
    for k in PARAMS:
        got = buffers(m)[k][:m.P]
        assert np.array_equal(bits(got).reshape(-1), R.bits(a[k]).reshape(-1)), f"{what}: {k} differs"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


# ---- pack -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,M,F", SHAPES)
def test_pack(hip, P, M, F):
    from online_lang_splatting_amd import map_io
    a, want = case(P, M, F)
    m = make_map(a, M, F, P + SPARE)
    rows = map_io.pack_rows(m)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (P, 14 + 3 * M + F) == want.shape
    got = bits(rows)
    assert not (got == np.int32(R.SENTINEL)).any(), "a word of the rows beyond P reached the record"
    bad = np.argwhere(got != R.bits(want))
    assert bad.size == 0, f"{len(bad)} words differ, the first at row {bad[0][0]}, column {bad[0][1]} ({map_io.attribute_names(M, F)[bad[0][1]]})"
    assert not got[:, 3:6].any(), "the normals are +0.0"
    assert_params(m, a, "the source after pack")


# ---- unpack -----------------------------------------------------------------------------------------------------------------
def file_layout(layout, want, M, F, seed):
    """(file body [P, n_cols] as float32 bits, col [width], the language the unpack must produce) for one layout of the file."""
    P, width = want.shape
    g = np.random.default_rng(seed)
    lang0 = 6 + 3 * M
    if layout == "plain":
        return want.copy(), list(range(width)), None
    if layout == "permuted":
        perm = g.permutation(width)                      # record column j lies in file column perm[j]
        body = np.empty_like(want)
        body[:, perm] = want
        return body, [int(c) for c in perm], None
    if layout == "extra":
        n_cols = width + 7                               # unknown columns between the known ones; the record's own are shuffled
        where = g.permutation(n_cols)[:width]
        body = R.random_bits((P, n_cols), seed + 1)
        body[:, where] = want
        col = [int(c) for c in where]
        col[3:6] = [-1, -1, -1]                          # the normals are never looked at
        return body, col, None
    assert layout == "no_language"
    keep = [j for j in range(width) if not lang0 <= j < lang0 + F]
    col = [-1] * width
    for c, j in enumerate(keep):
        col[j] = c
    return np.ascontiguousarray(want[:, keep]), col, np.zeros((P, F), dtype=np.float32)


@pytest.mark.parametrize("layout", ["plain", "permuted", "extra", "no_language"])
@pytest.mark.parametrize("P,M,F", SHAPES)
def test_unpack(hip, P, M, F, layout):
    from online_lang_splatting_amd._lib import check, lib
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    a, want = case(P, M, F)
    body, col, lang = file_layout(layout, want, M, F, seed=P + 7)
    m = GaussianMap.blank(P, M, F, LRS, DEV, capacity=P + SPARE)
    b = buffers(m)
    for k, v in b.items():
        if k != "cap":
            sentinel_fill(v)                              # every word of every destination buffer
    rows = torch.from_numpy(body).to(DEV)
    n_cols = body.shape[1]
    dst = m._struct(b)
    check(lib().olsr_map_ply_unpack(P, M, F, n_cols, (C.c_int32 * len(col))(*col), rows.data_ptr(), C.byref(dst), _stream()))
    torch.cuda.synchronize()
    expect = dict(a, language=lang) if lang is not None else a
    assert_params(m, expect, layout)
    for k, v in b.items():
        if k == "cap" or v.numel() == 0:
            continue
        tail = v[P:] if k in PARAMS else v               # parameters: the rows from P on; everything else: all of it
        assert bool((tail.reshape(-1).view(torch.int32) == R.SENTINEL).all()), f"{layout}: {k} was written outside rows [0, P)"
    assert np.array_equal(bits(rows), R.bits(body)), "the file's rows are only read"


# ---- files ------------------------------------------------------------------------------------------------------------------
ZERO_STATE = ("exp_avg", "exp_avg_sq", "stats", "max_radii", "kf_id", "n_obs")


def assert_fresh_state(m):
    st = m.state()
    for k in ZERO_STATE:
        assert st[k].shape[0] == m.P and not bool(st[k].reshape(-1).view(torch.int32).any()), f"{k} is not zero"
    assert m.group_steps == [0] * 7 and m.pending_skip == set()


@pytest.mark.parametrize("P,M,F", [(257, 4, 3), (513, 1, 32), (256, 1, 0)])
def test_file_round_trip(hip, tmp_path, P, M, F):
    from online_lang_splatting_amd import map_io
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    a, want = case(P, M, F)
    m = make_map(a, M, F, P + SPARE)
    m.kf_id.fill_(3)                                      # state the PLY does not carry
    m.stats.fill_(2.0)
    path = str(tmp_path / "deep" / "er" / "point_cloud.ply")
    m.save_ply(path)
    assert os.listdir(os.path.dirname(path)) == ["point_cloud.ply"], "the temporary file is gone"
    data = open(path, "rb").read()
    head = map_io.ply_header(P, M, F)
    assert data[:len(head)] == head and len(data) == len(head) + 4 * want.size
    # the tests' own reader
    names, body = R.read_ply(path)
    assert names == R.names_for(M, F) and np.array_equal(R.bits(body), R.bits(want))
    back = R.lookup(names, body, F)
    for k in PARAMS:
        assert np.array_equal(R.bits(back[k]).reshape(-1), R.bits(a[k]).reshape(-1)), k
    # load_ply
    ld = GaussianMap.load_ply(path, LRS, DEV)
    assert (ld.P, ld.M, ld.F) == (P, M, F) and ld.capacity >= P
    assert_params(ld, a, "load_ply")
    assert_fresh_state(ld)
    if F:
        no_lang = GaussianMap.load_ply(path, LRS, DEV, F=0, capacity=P + 5)
        assert (no_lang.P, no_lang.M, no_lang.F, no_lang.capacity) == (P, M, 0, P + 5) and no_lang.params["language"] is None
        assert_params(no_lang, dict(a, language=np.zeros((P, 0), dtype=np.float32)), "load_ply(F=0)")
        with pytest.raises(ValueError, match="language"):
            GaussianMap.load_ply(path, LRS, DEV, F=F - 1)
    else:
        zeros = GaussianMap.load_ply(path, LRS, DEV, F=15)   # a file without channels: zeros
        assert zeros.F == 15
        assert_params(zeros, dict(a, language=np.zeros((P, 15), dtype=np.float32)), "load_ply(F=15) of a file without channels")
    # saving over an existing file replaces it whole; a foreign file with other columns loads by name
    ld.save_ply(path)
    assert open(path, "rb").read() == data
    order = np.random.default_rng(5).permutation(len(names))
    foreign = str(tmp_path / "foreign.ply")
    R.write_ply(foreign, [names[i] for i in order] + ["confidence"],
                np.concatenate([body[:, order], R.random_bits((P, 1), 77)], axis=1), comments=["written by the test"])
    assert_params(GaussianMap.load_ply(foreign, LRS, DEV), a, "a permuted file with an unknown property")
    with pytest.raises(ValueError):
        GaussianMap(torch.zeros(4, 3), None, torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, 4), None, LRS, device=DEV).save_ply(path)


def test_empty_map(hip, tmp_path):
    from online_lang_splatting_amd import map_io
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    f32 = dict(dtype=torch.float32, device=DEV)
    m = GaussianMap(torch.zeros(0, 3, **f32), torch.zeros(0, 4, 3, **f32), torch.zeros(0, 1, **f32), torch.zeros(0, 3, **f32),
                    torch.zeros(0, 4, **f32), torch.zeros(0, 15, **f32), LRS, device=DEV)
    path = str(tmp_path / "empty.ply")
    m.save_ply(path)
    assert open(path, "rb").read() == map_io.ply_header(0, 4, 15)
    ld = GaussianMap.load_ply(path, LRS, DEV)
    assert (ld.P, ld.M, ld.F) == (0, 4, 15) and ld.params["means3D"].shape == (0, 3) and ld.capacity >= 1
    assert_fresh_state(ld)


def test_render_round_trip(hip, tmp_path):
    """A forward of a small scene from the loaded map equals the forward from the original bit for bit, in every output."""
    import parity_common as pc
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    from online_lang_splatting_amd.scene import Scene, make_scene
    sc = make_scene(3000, 64, 48, 15, seed=11, max_sh_degree=1)
    m = GaussianMap(sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations, sc.language, LRS, capacity=3000 + SPARE, device=DEV)
    path = str(tmp_path / "point_cloud.ply")
    m.save_ply(path)
    ld = GaussianMap.load_ply(path, LRS, DEV)

    def forward(gm):
        p = gm.params
        view = Scene(sc.camera, p["means3D"], p["opacities"], p["scales"], p["rotations"], p["shs"], p["language"], sc.sh_degree,
                     sc.bg, sc.F)
        fwd, _ = pc.run_forward(hip, view, DEV)
        torch.cuda.synchronize()
        return fwd
    a, b = forward(m), forward(ld)
    assert int(a["R"]) == int(b["R"]) > 0
    assert float(a["color"].abs().sum()) > 0 and int((a["radii"] > 0).sum()) > 1000, "the scene renders something"
    for k in ("color", "language", "depth", "opacity", "radii", "n_touched"):
        assert pc.same_bits(a[k], b[k]), f"{k} differs between the original and the loaded map"


# ---- the resumable state ----------------------------------------------------------------------------------------------------
def test_state_round_trip(hip, tmp_path):
    from online_lang_splatting_amd.frame_shard import GradientBucket
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    from online_lang_splatting_amd.scene import make_scene
    P, M, F = 700, 4, 15
    sc = make_scene(P, 64, 48, F, seed=5, max_sh_degree=1)
    drop = torch.rand(P, generator=torch.Generator().manual_seed(2)) < 0.3

    def bucket(m, seed):
        b = GradientBucket(m.P, m.layout, DEV)
        b.flat.copy_((torch.randn(m.P, m.layout.width, generator=torch.Generator().manual_seed(seed)) * 1e-3).to(DEV))
        return b

    def scenario(interrupt):
        m = GaussianMap(sc.means3D, sc.shs, torch.logit(sc.opacities), torch.log(sc.scales), sc.rotations, sc.language, LRS,
                        kf_id=torch.arange(P, dtype=torch.int32) % 5, n_obs=torch.arange(P, dtype=torch.int32) % 3, device=DEV)
        for s in range(3):
            assert m.step([bucket(m, s)]) == set()
        m.stats.copy_(torch.rand(P, 2, generator=torch.Generator().manual_seed(9)).to(DEV))
        m.max_radii.copy_(torch.arange(P, dtype=torch.int32).to(DEV))
        m.prune_points(drop)
        if interrupt:
            path = str(tmp_path / "run" / "map_state.npz")
            m.save_state(path)
            assert os.listdir(os.path.dirname(path)) == ["map_state.npz"]
            at_save = {k: v.clone() for k, v in m.state().items()}
            m = GaussianMap.load_state(path, LRS, DEV)
            for k, v in m.state().items():
                assert pc_same(v, at_save[k]), f"{k} differs right after load_state"
        skipped = [m.step([bucket(m, 3 + s)]) for s in range(2)]
        assert len(skipped[0]) == 7 and skipped[1] == set(), "the step after an edit skips every group, also after a resume"
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in m.state().items()}
    whole, resumed = scenario(False), scenario(True)
    assert whole["means3D"].shape[0] == int((~drop).sum()) and whole["group_steps"].tolist() == [4] * 7
    for k in whole:
        assert pc_same(whole[k], resumed[k]), f"{k} differs between the uninterrupted and the resumed map"


def pc_same(a, b):
    import parity_common as pc
    return pc.same_bits(a, b)


# ---- the session ------------------------------------------------------------------------------------------------------------
def test_session_save_gaussians(hip, tmp_path):
    """One frame through OnlineSlam.track (initialisation only, 6 iterations), then the two paths of save_gaussians."""
    import test_gpu_online_slam as T
    from online_lang_splatting_amd import OnlineSlam
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    from online_lang_splatting_amd.scene import _raycast_room, _room_colour, _surface_codes, world2view2
    cam = T.path_cameras()[0]
    depth, hitp, sid = _raycast_room(cam, T.W, T.H)        # frame 0, as T.make_sequence builds it
    rgb = (_room_colour(hitp, sid) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous().to(DEV)
    d16 = (depth.double() * T.DEPTH_SCALE).round().clamp(0, 65535).to(torch.int32).numpy().astype(np.uint16)
    _, _, sid_l = _raycast_room(cam, 48, 32)
    codes = _surface_codes(T.F)[sid_l].permute(2, 0, 1).contiguous().to(DEV)
    fx = T.W / 2.0
    slam = OnlineSlam(T.config(init_itr_num=6), (fx, fx, (T.W - 1) / 2.0, (T.H - 1) / 2.0), T.H, T.W,
                      feature_fn=lambda i, image: codes, device=DEV)
    assert slam.save_gaussians(None, final=True) is None
    r = slam.track(0, rgb, torch.from_numpy(d16).to(DEV), T.DEPTH_SCALE, gt_w2c=world2view2(cam.R, cam.T))
    assert r["is_keyframe"] and slam.map.P > 100 and slam.map.F == T.F
    out = tmp_path / "results"
    assert slam.save_gaussians(None, iteration=7) is None and not out.exists(), "save_dir=None writes nothing"
    p7 = slam.save_gaussians(str(out), iteration=7)
    pf = slam.save_gaussians(str(out), final=True)
    assert p7 == str(out / "point_cloud" / "iteration_7" / "point_cloud.ply") and os.path.isfile(p7)
    assert pf == str(out / "point_cloud" / "final" / "point_cloud.ply") and os.path.isfile(pf)
    assert sorted(os.listdir(out / "point_cloud")) == ["final", "iteration_7"]
    want = {k: (v.detach().cpu().numpy() if v is not None else np.zeros((slam.map.P, 0), np.float32))
            for k, v in slam.map.params.items()}
    for path in (p7, pf):
        ld = GaussianMap.load_ply(path, slam.lrs, DEV)
        assert (ld.P, ld.M, ld.F) == (slam.map.P, slam.map.M, slam.map.F)
        assert_params(ld, want, path)
