"""Host side of olsr_tsdf_* (include/olsr.h): TSDF fusion of depth and language maps into a 3-D map, on the device.

Counterpart of the reference's tsdf-fusion/fusion.py (packed 8-bit colour), fusion2.py (3 float channels) and fusion3.py (15
float channels, what tsdf-fusion/dim15_recon.py fuses): `TSDFVolume(vol_bnds, voxel_size)` with `integrate(color_im, depth_im,
cam_intr, cam_pose, obs_weight)`, `get_volume()` and `get_point_cloud()`.  The volume lives on the GPU, rendered maps go in as
the device tensors the rasteriser returned (integrate_render), several views are fused in one launch (integrate_views), and
the surface comes from the device as well.  get_point_cloud returns the zero crossings of the grid edges — the edge vertices
of marching cubes at level 0; get_mesh returns the same vertices with faces and normals, the triangles from a generated table
(scripts/gen_mc_table.py) without Lewiner's interior vertices: no parity with skimage's vertex order, faces or winding is
claimed.  meshwrite, meshwrite_color and pcwrite write the ASCII PLY files of fusion3.py (tsdf-fusion/dim15_recon.py:86-97), which
the reference's 3-D evaluation reads back.  GPU only; there is no torch fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._host import require_gpu_device, stream_ptr
from ._lib import check, lib

COLOR_CONST = 256 * 256


def rigid_transform(xyz, transform):
    """[N,3] points through a 4 x 4 transform (host, float64)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    T = np.asarray(transform, dtype=np.float64)
    return xyz @ T[:3, :3].T + T[:3, 3]


def get_view_frustum(depth_im, cam_intr, cam_pose):
    """The five corners [3,5] of a depth image's view frustum in the world: the camera centre and the image corners at the
    largest depth (fusion.py get_view_frustum).  Host arithmetic; depth_im may be a device tensor (one scalar is read back)."""
    h, w = int(depth_im.shape[0]), int(depth_im.shape[1])
    max_depth = float(depth_im.max())
    K = np.asarray(cam_intr, dtype=np.float64)
    u = np.array([0.0, 0.0, 0.0, w, w])
    v = np.array([0.0, 0.0, h, 0.0, h])
    z = np.array([0.0, max_depth, max_depth, max_depth, max_depth])
    pts = np.stack([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z], axis=1)
    return rigid_transform(pts, cam_pose).T


def _host(name, a, shape):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    if a.shape != shape:
        raise RuntimeError(f"{name} has shape {tuple(a.shape)}, expected {shape}")
    return a


class TSDFVolume:
    """A TSDF volume with per-voxel features on `device`.

    feature_dim: 0 (geometry only), 3, 15, 16 or 32 float channels, each the weighted running mean of its observations
    (fusion2.py / fusion3.py), or "rgb": the packed 8-bit colour of fusion.py.  Constructor arithmetic as in the reference
    (fusion.py:30-42), except that the caller's vol_bnds array is not modified."""

    def __init__(self, vol_bnds, voxel_size, feature_dim=15, device="cuda"):
        self.device = require_gpu_device(device, "TSDFVolume")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        bnds = np.array(vol_bnds, dtype=np.float64)
        if bnds.shape != (3, 2):
            raise RuntimeError(f"TSDFVolume: vol_bnds has shape {tuple(bnds.shape)}, expected (3, 2)")
        self.packed = feature_dim == "rgb"
        if not self.packed and feature_dim not in _abi.SUPPORTED_F:
            raise RuntimeError(f"TSDFVolume: feature_dim must be \"rgb\" or one of {_abi.SUPPORTED_F}, got {feature_dim!r}")
        self.feature_dim = 3 if self.packed else int(feature_dim)   # channels of an input image and of a surface point
        self._voxel_size = float(voxel_size)
        if not self._voxel_size > 0.0:
            raise RuntimeError(f"TSDFVolume: voxel_size must be positive, got {voxel_size}")
        self._trunc_margin = 5 * self._voxel_size
        self._vol_dim = np.ceil((bnds[:, 1] - bnds[:, 0]) / self._voxel_size).copy(order="C").astype(int)
        if int(self._vol_dim.min()) < 1:
            raise RuntimeError(f"TSDFVolume: vol_bnds gives an empty volume {self._vol_dim.tolist()}")
        bnds[:, 1] = bnds[:, 0] + self._vol_dim * self._voxel_size
        self._vol_bnds = bnds
        self._vol_origin = bnds[:, 0].copy(order="C").astype(np.float32)
        X, Y, Z = (int(d) for d in self._vol_dim)
        if X * Y * Z >= 1 << 31:
            raise RuntimeError(f"TSDFVolume: {X} x {Y} x {Z} voxels, fewer than 2^31 are supported")
        planes = 1 if self.packed else self.feature_dim
        self._tsdf = torch.empty((X, Y, Z), dtype=torch.float32, device=self.device)
        self._weight = torch.empty((X, Y, Z), dtype=torch.float32, device=self.device)
        self._feat = torch.empty((X, Y, Z) if self.packed else (planes, X, Y, Z), dtype=torch.float32, device=self.device)
        self._vol = _abi.OlsrTsdfVolume(X=X, Y=Y, Z=Z, F=planes,
                                        feat_mode=_abi.TSDF_FEAT_PACKED_RGB if self.packed else _abi.TSDF_FEAT_FLOAT,
                                        voxel_size=self._voxel_size, trunc_margin=self._trunc_margin,
                                        tsdf=self._tsdf.data_ptr(), weight=self._weight.data_ptr(),
                                        feat=self._feat.data_ptr() if planes > 0 else None)
        for k in range(3):
            self._vol.origin[k] = float(self._vol_origin[k])
        self._scratch = None
        self._status = torch.zeros(4, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().olsr_tsdf_init(C.byref(self._vol), stream_ptr(self.device)))

    # ---- what the reference's attributes hold ----------------------------------------------------------------------------
    @property
    def vol_dim(self):
        return tuple(int(d) for d in self._vol_dim)

    @property
    def vol_bnds(self):
        return self._vol_bnds.copy()

    @property
    def vol_origin(self):
        return self._vol_origin.copy()

    @property
    def voxel_size(self):
        return self._voxel_size

    @property
    def trunc_margin(self):
        return self._trunc_margin


    # ---- one view ----------------------------------------------------------------------------------------------------------
    def _image(self, who, name, t, shapes):
        """A float32 device tensor of one of `shapes`, as it is; a numpy array is uploaded."""
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(self.device)
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be a float32 tensor on the GPU or a numpy array")
        if t.device != self.device:
            raise RuntimeError(f"{who}: {name} is on {t.device}, expected {self.device}")
        if tuple(t.shape) not in shapes:
            raise RuntimeError(f"{who}: {name} has shape {tuple(t.shape)}, expected " + " or ".join(str(list(s)) for s in shapes))
        return t.detach().contiguous()

    def _view(self, who, color_im, depth_im, cam_intr, cam_pose, obs_weight=1., opacity=None, min_opacity=0.0, layout=None):
        """-> (olsr_tsdf_view, the tensors it points to)."""
        if isinstance(depth_im, (np.ndarray, torch.Tensor)) and depth_im.ndim == 3 and depth_im.shape[0] == 1:
            depth_im = depth_im[0]   # the rasteriser's [1,H,W]
        if not isinstance(depth_im, (np.ndarray, torch.Tensor)) or depth_im.ndim != 2 or min(depth_im.shape) < 1:
            raise RuntimeError(f"{who}: depth_im must be an [H,W] image, got {getattr(depth_im, 'shape', type(depth_im).__name__)}")
        H, W = int(depth_im.shape[0]), int(depth_im.shape[1])
        depth = self._image(who, "depth_im", depth_im, [(H, W)])
        F = self.feature_dim
        feat, lay = None, _abi.TSDF_IMAGE_CHANNELS
        if F > 0:
            if color_im is None:
                raise RuntimeError(f"{who}: color_im is required (the volume has {F} feature channels)")
            if layout not in (None, "channels", "rows"):
                raise RuntimeError(f"{who}: layout must be \"channels\" ([F,H,W]) or \"rows\" ([H,W,F]), got {layout!r}")
            if self.packed:
                if isinstance(color_im, np.ndarray):
                    color_im = torch.from_numpy(np.ascontiguousarray(color_im).astype(np.float32)).to(self.device)
                elif isinstance(color_im, torch.Tensor) and color_im.is_cuda and color_im.dtype == torch.uint8:
                    color_im = color_im.float()
                rgb = self._image(who, "color_im", color_im, [(H, W, 3)])
                # fold the colour into one channel (fusion.py:221-222)
                feat = torch.floor(rgb[..., 2] * COLOR_CONST + rgb[..., 1] * 256 + rgb[..., 0]).contiguous()
            else:
                if isinstance(color_im, np.ndarray):
                    layout = layout or "rows"   # the reference's (H, W, F) arrays
                shapes = {"channels": (F, H, W), "rows": (H, W, F)}
                feat = self._image(who, "color_im", color_im, [shapes[layout]] if layout else list(shapes.values()))
                if layout is None:
                    if shapes["channels"] == shapes["rows"]:
                        raise RuntimeError(f"{who}: color_im of shape {tuple(feat.shape)} is ambiguous, pass layout=")
                    layout = "channels" if tuple(feat.shape) == shapes["channels"] else "rows"
                lay = _abi.TSDF_IMAGE_CHANNELS if layout == "channels" else _abi.TSDF_IMAGE_ROWS
        opa = None
        if opacity is not None:
            if isinstance(opacity, (np.ndarray, torch.Tensor)) and opacity.ndim == 3 and opacity.shape[0] == 1:
                opacity = opacity[0]
            opa = self._image(who, "opacity", opacity, [(H, W)])
        K, pose = _host(f"{who}: cam_intr", cam_intr, (3, 3)), _host(f"{who}: cam_pose", cam_pose, (4, 4))
        v = _abi.OlsrTsdfView(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], obs_weight=float(obs_weight),
                              min_opacity=float(min_opacity), H=H, W=W, feat_layout=lay, depth=depth.data_ptr(),
                              feat=None if feat is None else feat.data_ptr(), opacity=None if opa is None else opa.data_ptr())
        for k, x in enumerate(pose.astype(np.float32).reshape(-1)):
            v.pose[k] = float(x)
        return v, (depth, feat, opa)

    def _launch(self, views):
        L = lib()
        with torch.cuda.device(self.device):
            for s in range(0, len(views), _abi.TSDF_MAX_VIEWS):
                chunk = views[s:s + _abi.TSDF_MAX_VIEWS]
                arr = (_abi.OlsrTsdfView * len(chunk))(*[v for v, _ in chunk])
                check(L.olsr_tsdf_integrate(C.byref(self._vol), len(chunk), arr, stream_ptr(self.device)))

    def integrate(self, color_im, depth_im, cam_intr, cam_pose, obs_weight=1., opacity=None, min_opacity=0.0, layout=None):
        """Fuses one frame (the reference's signature).  color_im: [H,W,F] (numpy, as in the reference, or a device tensor) or
        a device tensor [F,H,W]; "rgb" volumes take [H,W,3] with values 0..255; F = 0 volumes ignore it.  depth_im [H,W], 0 =
        invalid; cam_intr [3,3]; cam_pose [4,4] camera to world.  opacity [H,W] with min_opacity masks pixels below it."""
        self._launch([self._view("integrate", color_im, depth_im, cam_intr, cam_pose, obs_weight, opacity, min_opacity, layout)])

    def integrate_views(self, views):
        """Fuses a list of frames, OLSR_TSDF_MAX_VIEWS per launch, in order: the result equals integrate() per frame bit for
        bit, with one read and one write of the touched voxels per launch.  A frame is a tuple in integrate()'s argument
        order or a dict of its arguments."""
        built = []
        for k, f in enumerate(views):
            who = f"integrate_views[{k}]"
            if isinstance(f, dict):
                built.append(self._view(who, **f))
            elif isinstance(f, (tuple, list)) and 4 <= len(f) <= 8:
                built.append(self._view(who, *f))
            else:
                raise RuntimeError(f"{who}: a tuple (color_im, depth_im, cam_intr, cam_pose[, obs_weight, ...]) or a dict is expected")
        if built:
            self._launch(built)

    @staticmethod
    def render_view(render_pkg, cam_intr, w2c, depth=None, min_opacity=0.5, obs_weight=1.):
        """The frame dict integrate_views takes, from render(...)'s result: its "language" [F,H,W] (or "render" for an "rgb" /
        3-channel volume when there is no language map), "depth" and "opacity" as they are on the device.  w2c [4,4]: world
        to camera.  depth: a sensor depth image [H,W] to fuse in place of the rendered one (what the reference fuses); the
        opacity mask then applies to it as well unless min_opacity is 0."""
        if not isinstance(render_pkg, dict) or "depth" not in render_pkg:
            raise RuntimeError("integrate_render: the dict render(...) returns is expected")
        color = render_pkg.get("language")
        if color is None:
            color = render_pkg.get("render")
        pose = np.linalg.inv(_host("integrate_render: w2c", w2c, (4, 4)))
        opacity = render_pkg.get("opacity") if min_opacity > 0 else None
        return dict(color_im=None if color is None else color.detach(), depth_im=render_pkg["depth"].detach() if depth is None else depth,
                    cam_intr=cam_intr, cam_pose=pose, obs_weight=obs_weight, opacity=None if opacity is None else opacity.detach(),
                    min_opacity=min_opacity, layout="channels")

    def integrate_render(self, render_pkg, cam_intr, w2c, depth=None, min_opacity=0.5, obs_weight=1.):
        """Fuses render(...)'s language and depth maps with no host copy (see render_view)."""
        f = self.render_view(render_pkg, cam_intr, w2c, depth, min_opacity, obs_weight)
        if self.feature_dim == 0:
            f["color_im"] = None
        self._launch([self._view("integrate_render", **f)])

    # ---- results -----------------------------------------------------------------------------------------------------------
    def get_volume(self):
        """(tsdf [X,Y,Z], features): the features are [F,X,Y,Z] (None for F = 0), or the packed colour [X,Y,Z] of an "rgb"
        volume.  The tensors are the volume itself, not copies."""
        return self._tsdf, (self._feat if self.feature_dim > 0 else None)

    @property
    def weight(self):
        return self._weight

    def surface_points(self, min_weight=0.0):
        """-> (points [N,3] world coordinates, feats [N,F] or None, voxel_index int32 [N]): one point per grid edge on which
        the distance changes sign, its features those of the nearest voxel, in voxel order then axis (x, y, z).  min_weight >
        0 keeps only edges whose two voxels have at least that weight; 0 is the reference, where an unobserved voxel is +1."""
        L = lib()
        X, Y, Z = self.vol_dim
        nbytes = L.olsr_tsdf_surface_scratch_bytes(X, Y, Z)
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(L.olsr_tsdf_surface_plan(C.byref(self._vol), float(min_weight), self._scratch.data_ptr(),
                                           self._status.data_ptr(), stream_ptr(self.device)))
            n = int(self._status[0].item())   # the extraction's one host synchronisation
            F = self.feature_dim
            points = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            feats = torch.empty((n, F), dtype=torch.float32, device=self.device) if F > 0 else None
            index = torch.empty((n,), dtype=torch.int32, device=self.device)
            check(L.olsr_tsdf_surface_emit(C.byref(self._vol), float(min_weight), self._scratch.data_ptr(), n,
                                           points.data_ptr() if n else None, feats.data_ptr() if F > 0 and n else None,
                                           index.data_ptr() if n else None, stream_ptr(self.device)))
        return points, feats, index

    def get_mesh(self, min_weight=0.0):
        """-> (verts [N,3], faces int32 [M,3], norms [N,3], colors [N,F] or None), the reference's order, on the device.  The
        vertices and colours are surface_points' (same order, same bits); a face (i, j, k) indexes them, wound so that
        cross(v_j - v_i, v_k - v_i) points to free space, as the per-vertex normals do (the normalised gradient of the
        distance).  min_weight > 0 triangulates only cubes whose eight voxels have at least that weight.  One host read of 16
        bytes."""
        return self._mesh(min_weight)[:4]

    def _mesh(self, min_weight):
        """get_mesh's tuple and voxel_index int32 [N], the owner of every vertex as surface_points returns it."""
        L = lib()
        X, Y, Z = self.vol_dim
        nbytes = L.olsr_tsdf_mesh_scratch_bytes(X, Y, Z)
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(L.olsr_tsdf_mesh_plan(C.byref(self._vol), float(min_weight), self._scratch.data_ptr(),
                                        self._status.data_ptr(), stream_ptr(self.device)))
            n, m = self._status.tolist()[:2]   # the extraction's one host synchronisation: 16 bytes
            if m > (2 ** 31 - 1) // 3:
                raise RuntimeError(f"get_mesh: {m} or more faces, 3 * faces must stay below 2^31")
            F = self.feature_dim
            verts = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            norms = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            colors = torch.empty((n, F), dtype=torch.float32, device=self.device) if F > 0 else None
            faces = torch.empty((m, 3), dtype=torch.int32, device=self.device)
            index = torch.empty((n,), dtype=torch.int32, device=self.device)
            check(L.olsr_tsdf_mesh_emit(C.byref(self._vol), float(min_weight), self._scratch.data_ptr(), n, m,
                                        verts.data_ptr() if n else None, norms.data_ptr() if n else None,
                                        colors.data_ptr() if F > 0 and n else None, index.data_ptr() if n else None,
                                        faces.data_ptr() if m else None, stream_ptr(self.device)))
        return verts, faces, norms, colors, index

    def get_point_cloud(self, min_weight=0.0):
        """[N,3+F]: surface_points' points and features side by side (an "rgb" volume: x, y, z, r, g, b as floats)."""
        points, feats, _ = self.surface_points(min_weight)
        return points if feats is None else torch.cat([points, feats], dim=1)

    get_view_frustum = staticmethod(get_view_frustum)


# ---- the PLY files of the reference's 3-D evaluation (fusion3.py meshwrite, meshwrite_color, pcwrite) ---------------------------
_FEATURE_NAMES = ("red", "green", "blue") + tuple(f"f{k}" for k in range(4, 16))


def _array(name, a, cols, dtype=np.float64):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2 or (cols is not None and a.shape[1] < cols):
        raise RuntimeError(f"{name} has shape {tuple(a.shape)}, expected [N,{cols if cols is not None else 'C'}]")
    return a if dtype is None else a.astype(dtype)


def _write_ply(filename, vertex_properties, rows, faces=None):
    lines = ["ply", "format ascii 1.0", f"element vertex {len(rows)}"] + [f"property {p}" for p in vertex_properties]
    if faces is not None:
        lines += [f"element face {len(faces)}", "property list uchar int vertex_index"]
    lines.append("end_header")
    lines += rows
    if faces is not None:
        lines += ["3 %d %d %d" % (f[0], f[1], f[2]) for f in faces.tolist()]
    with open(filename, "w") as f:
        f.write("\n".join(lines) + "\n")


def _mesh_arrays(who, verts, faces, norms, colors, n_colors):
    verts, norms = _array(f"{who}: verts", verts, 3), _array(f"{who}: norms", norms, 3)
    faces = _array(f"{who}: faces", faces, 3, np.int64)
    colors = _array(f"{who}: colors", colors, n_colors, None)
    if not (len(verts) == len(norms) == len(colors)):
        raise RuntimeError(f"{who}: {len(verts)} verts, {len(norms)} norms and {len(colors)} colors")
    return verts, faces, norms, colors


def meshwrite(filename, verts, faces, norms, colors):
    """The 15-feature mesh (semantic_mesh.ply): x y z nx ny nz and the features as floats named red, green, blue, f4 ... f15,
    every number as "%f"; then "3 i j k" per face.  Tensors or arrays."""
    verts, faces, norms, colors = _mesh_arrays("meshwrite", verts, faces, norms, colors, 15)
    fmt = " ".join(["%f"] * 21)
    rows = [fmt % tuple(r) for r in np.concatenate([verts, norms, colors[:, :15].astype(np.float64)], axis=1).tolist()]
    _write_ply(filename, [f"float {n}" for n in ("x", "y", "z", "nx", "ny", "nz") + _FEATURE_NAMES], rows, faces)


def meshwrite_color(filename, verts, faces, norms, colors):
    """The coloured mesh (semantic_mesh_color.ply, one per queried class): x y z nx ny nz as "%f" and the first three colour
    columns converted to uint8, "%d"."""
    verts, faces, norms, colors = _mesh_arrays("meshwrite_color", verts, faces, norms, colors, 3)
    rgb = colors.astype(np.uint8)
    fmt = " ".join(["%f"] * 6 + ["%d"] * 3)
    rows = [fmt % (tuple(a) + tuple(b)) for a, b in zip(np.concatenate([verts, norms], axis=1).tolist(), rgb[:, :3].tolist())]
    _write_ply(filename, [f"float {n}" for n in ("x", "y", "z", "nx", "ny", "nz")] + [f"uchar {n}" for n in _FEATURE_NAMES[:3]],
               rows, faces)


def pcwrite(filename, xyzfeat):
    """The 15-feature point cloud (semantic_pc.ply) from get_point_cloud's [N,18]: x y z and the features, "%f"."""
    a = _array("pcwrite: xyzfeat", xyzfeat, 18)
    fmt = " ".join(["%f"] * 18)
    _write_ply(filename, [f"float {n}" for n in ("x", "y", "z") + _FEATURE_NAMES], [fmt % tuple(r) for r in a[:, :18].tolist()])


def label_points(query, feats):
    """Semantic label per surface point, [N] int64: the reference's get_semantic_map_pc
    (tsdf-fusion/3d_evaluation_and_visualize_langslam_dim15.py:103-115) — decode the points' 15-channel codes, take the products
    with the label embeddings, argmax (the softmax in between is monotone).  `query`: a LanguageQuery with set_phrases and
    set_labels done; feats [N,15] as surface_points returns them."""
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda or feats.dtype != torch.float32:
        raise RuntimeError("label_points: feats must be a float32 tensor on the GPU")
    if feats.dim() != 2 or feats.shape[1] != _abi.LANG_AE_CODE:
        raise RuntimeError(f"label_points: feats has shape {tuple(feats.shape)}, expected [N,{_abi.LANG_AE_CODE}]")
    n_pos, n_lab, _ = query.counts
    if n_lab < 1:
        raise RuntimeError("label_points: set_labels first")
    if feats.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=feats.device)
    sims = query.similarities(feats.t().contiguous())   # [K,1,N]
    return torch.argmax(sims[n_pos:n_pos + n_lab, 0, :], dim=0)


TSDFVolume.label_points = staticmethod(label_points)
