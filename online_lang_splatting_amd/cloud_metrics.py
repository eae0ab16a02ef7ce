"""Host side of olsr_emd_cost and olsr_chamfer (include/olsr.h): the two numbers the reference's 3-D evaluation reports per
queried class (tsdf-fusion/3d_evaluation_and_visualize_langslam_dim15.py:396-423), on the device.

`earth_mover_distance` and `chamfer_distance` keep the reference's signatures (tsdf-fusion/emd.py; :235-274 of the evaluation
script, metric 'l2').  `emd_segments` and `chamfer_segments` are the ragged forms behind them: B pairs of clouds, packed
[total,3] arrays with [B+1] offsets, all pairs in the same launches.  `evaluate_classes` is the evaluation's loop over the
queried classes with one batched call of each and one host read.

Chamfer is brute force: its cost grows as n * m per segment; a spatial grid is out of scope.  The EMD is PyTorchEMD's
approximate matching without the match matrix: the reference fills a dense [m,n] matrix only to form sum d * match from it,
and the copy of emd.py the evaluation uses keeps nothing for a backward, so neither the matrix nor a backward is offered here;
memory is O(n + m).  GPU only; there is no torch fallback.
"""
import numpy as np
import torch

from . import _abi
from ._host import ptr, scratch_for, stream_ptr
from ._lib import check, lib


def _points(who, name, t, device=None):
    """A float32 [N,3] device tensor, contiguous."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{who}: {name} must be a tensor on the GPU (there is no torch fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{who}: {name} must be float32, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{who}: {name} has shape {tuple(t.shape)}, expected [N,3]")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a tensor on the GPU (there is no torch fallback)")
    if device is not None and t.device != device:
        raise RuntimeError(f"{who}: {name} is on {t.device}, expected {device}")
    return t.detach().contiguous()


def _offsets(who, name, off, total):
    """int32 [B+1] on the host (a device tensor costs one read: the longest segment sizes the grid)."""
    if isinstance(off, torch.Tensor):
        if off.dtype not in (torch.int32, torch.int64):
            raise RuntimeError(f"{who}: {name} must be an integer tensor, got {off.dtype}")
        off = off.detach().cpu().numpy()
    off = np.asarray(off)
    if off.ndim != 1 or off.size < 2 or not np.issubdtype(off.dtype, np.integer):
        raise RuntimeError(f"{who}: {name} must be B + 1 >= 2 integers, got shape {tuple(off.shape)} of {off.dtype}")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off[0] < 0 or np.any(np.diff(off) < 0):
        raise RuntimeError(f"{who}: {name} must start at >= 0 and not decrease")
    if off[-1] > total:
        raise RuntimeError(f"{who}: {name} ends at {int(off[-1])}, but there are {total} points")
    if off[-1] >= (1 << 31) // 3:
        raise RuntimeError(f"{who}: {name} ends at {int(off[-1])}, fewer than 2^31 / 3 points are supported")
    return off.astype(np.int32)


def _segments(who, xyz1, off1, xyz2, off2, names=("xyz1", "off1", "xyz2", "off2")):
    xyz1 = _points(who, names[0], xyz1)
    xyz2 = _points(who, names[2], xyz2, xyz1.device)
    off1 = _offsets(who, names[1], off1, xyz1.shape[0])
    off2 = _offsets(who, names[3], off2, xyz2.shape[0])
    if off1.size != off2.size:
        raise RuntimeError(f"{who}: {names[1]} describes {off1.size - 1} segments, {names[3]} {off2.size - 1}")
    B = off1.size - 1
    if B > _abi.CLOUD_MAX_SEGMENTS:
        raise RuntimeError(f"{who}: {B} segments, at most {_abi.CLOUD_MAX_SEGMENTS} are supported")
    return xyz1, off1, xyz2, off2, B, int(np.diff(off1).max()), int(np.diff(off2).max())


def _emd(who, xyz1, off1, xyz2, off2):
    """-> (cost [B] float64, undivided; residual [B,2] float32; valid [B] int32; n1 [B] as a host array)."""
    xyz1, off1, xyz2, off2, B, max1, max2 = _segments(who, xyz1, off1, xyz2, off2)
    dev = xyz1.device
    L = lib()
    scratch = scratch_for(dev, "emd", L.olsr_emd_scratch_bytes(B, int(off1[-1]), int(off2[-1])))
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    residual = torch.empty((B, 2), dtype=torch.float32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.olsr_emd_cost(B, off1.ctypes.data, off2.ctypes.data, max1, max2, ptr(xyz1), ptr(xyz2),
                              cost.data_ptr(), residual.data_ptr(), valid.data_ptr(), scratch.data_ptr(), stream_ptr(dev)))
    return cost, residual, valid, np.diff(off1)


def emd_segments(xyz1, off1, xyz2, off2, return_residual=False):
    """The approximate earth mover's distance of B pairs of clouds: segment b is xyz1[off1[b]:off1[b+1]] against
    xyz2[off2[b]:off2[b+1]].  xyz1 [total1,3], xyz2 [total2,3]: float32 on the GPU; off1, off2: B + 1 integers (a list, an
    array or a tensor).  -> emd [B] float64, the matching's cost divided by the segment's n1, NaN where a side is empty; with
    return_residual also residual [B,2] float32: the mass of cloud 1 and of cloud 2 the matching left unassigned (out of
    max(n1, n2)), which the reference drops silently — how far to trust the number."""
    cost, residual, _, n1 = _emd("emd_segments", xyz1, off1, xyz2, off2)
    emd = cost / torch.from_numpy(np.maximum(n1, 1).astype(np.float64)).to(cost.device)
    return (emd, residual) if return_residual else emd


def _batched(who, name, t):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{who}: {name} must be a tensor on the GPU (there is no torch fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{who}: {name} must be float32, got {t.dtype}")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise RuntimeError(f"{who}: {name} has shape {tuple(t.shape)}, expected (b, 3, n), or (b, n, 3) with transpose=False")
    return t


def earth_mover_distance(xyz1, xyz2, transpose=True):
    """The reference's earth_mover_distance (tsdf-fusion/emd.py): xyz1 (b, 3, n1), xyz2 (b, 3, n2), or (b, n, 3) with
    transpose=False; 2-D inputs get a batch axis.  -> (b,) float32: the approximate matching's cost divided by n1.
    No match matrix and no backward (see the module's docstring)."""
    who = "earth_mover_distance"
    xyz1, xyz2 = _batched(who, "xyz1", xyz1), _batched(who, "xyz2", xyz2)
    if transpose:
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
    if xyz1.shape[2] != 3 or xyz2.shape[2] != 3:
        raise RuntimeError(f"{who}: xyz1 {tuple(xyz1.shape)} and xyz2 {tuple(xyz2.shape)} must be (b, n, 3) after the transpose")
    if xyz1.shape[0] != xyz2.shape[0]:
        raise RuntimeError(f"{who}: xyz1 has a batch of {xyz1.shape[0]}, xyz2 of {xyz2.shape[0]}")
    b, n1, n2 = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if b < 1:
        raise RuntimeError(f"{who}: the batch is empty")
    if not xyz1.is_cuda or not xyz2.is_cuda:
        raise RuntimeError(f"{who}: xyz1 and xyz2 must be tensors on the GPU (there is no torch fallback)")
    emd = emd_segments(xyz1.reshape(b * n1, 3), np.arange(b + 1) * n1, xyz2.reshape(b * n2, 3), np.arange(b + 1) * n2)
    return emd.float()


def chamfer_segments(x, offx, y, offy):
    """Chamfer distances of B pairs of clouds (segments as in emd_segments).  -> (mean [B,2] float64, min_d2_x [total_x]
    float32, nn_x [total_x] int32, min_d2_y, nn_y): mean[b] = (mean over x of the distance to the nearest y, mean over y of the
    distance to the nearest x), NaN where a side is empty; per point the SQUARED distance to its nearest point of the other
    cloud of its segment and that point's index inside the segment (the lowest on ties).  Brute force, n * m per segment."""
    who = "chamfer_segments"
    x, offx, y, offy, B, maxx, maxy = _segments(who, x, offx, y, offy, ("x", "offx", "y", "offy"))
    dev = x.device
    L = lib()
    scratch = scratch_for(dev, "chamfer", L.olsr_chamfer_scratch_bytes(B, int(offx[-1]), int(offy[-1])))
    mean = torch.empty((B, 2), dtype=torch.float64, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    # (points no segment covers keep these values)
    dx = torch.full((x.shape[0],), float("nan"), dtype=torch.float32, device=dev)
    dy = torch.full((y.shape[0],), float("nan"), dtype=torch.float32, device=dev)
    ix = torch.full((x.shape[0],), -1, dtype=torch.int32, device=dev)
    iy = torch.full((y.shape[0],), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.olsr_chamfer(B, offx.ctypes.data, offy.ctypes.data, maxx, maxy, ptr(x), ptr(y),
                             ptr(dx), ptr(ix), ptr(dy), ptr(iy), mean.data_ptr(), valid.data_ptr(), scratch.data_ptr(),
                             stream_ptr(dev)))
    return mean, dx, ix, dy, iy


def _direction(who, mean, direction):
    if direction == "x_to_y":
        return mean[:, 0]
    if direction == "y_to_x":
        return mean[:, 1]
    if direction == "bi":
        return mean[:, 1] + mean[:, 0]   # the reference's order of the two terms
    raise RuntimeError(f"{who}: direction must be 'y_to_x', 'x_to_y' or 'bi', got {direction!r}")


def chamfer_distance(x, y, direction="bi"):
    """The reference's chamfer_distance (metric 'l2'): x [n,3], y [m,3], float32 on the GPU.  'y_to_x': the mean over y of the
    Euclidean distance (not squared) to the nearest x; 'x_to_y': the converse; 'bi': their sum.  -> a float64 scalar tensor on
    the device (the result is not read back); NaN if a cloud is empty.  Brute force: the cost grows as n * m."""
    who = "chamfer_distance"
    _direction(who, torch.zeros((1, 2)), direction)
    x, y = _points(who, "x", x), _points(who, "y", y)
    mean = chamfer_segments(x, [0, x.shape[0]], y, [0, y.shape[0]])[0]
    return _direction(who, mean, direction)[0]


def evaluate_classes(points, labels, gt_points, gt_labels, pairs, stride=8):
    """The evaluation's loop over the queried classes (:396-423).  points [N,3] float32 with labels [N] (what
    tsdf.label_points returns), gt_points [M,3] with gt_labels [M], all on the GPU; pairs: (pred_id, gt_id) per query (matching
    the ground truth's colours to class ids stays with the caller).  Per query the clouds are points[labels == pred_id][::stride]
    and gt_points[gt_labels == gt_id][::stride]; all queries then share one Chamfer call and one EMD call and one host read.
    -> (per query a dict n_pred, n_gt, cd ('bi'), emd, emd_residual (left, right), or None where a side is empty — the
    reference `continue`s; {"cd", "emd": the averages over the evaluated queries as the reference prints them, None if there
    is none, "evaluated": their number})."""
    who = "evaluate_classes"
    points, gt_points = _points(who, "points", points), _points(who, "gt_points", gt_points)
    for name, lab, pts in (("labels", labels, points), ("gt_labels", gt_labels, gt_points)):
        if not isinstance(lab, torch.Tensor) or lab.device != pts.device or lab.dim() != 1 or lab.shape[0] != pts.shape[0]:
            raise RuntimeError(f"{who}: {name} must be an [N] tensor on the device of its points, one label per point")
        if lab.dtype.is_floating_point or lab.dtype == torch.bool:
            raise RuntimeError(f"{who}: {name} must be an integer tensor, got {lab.dtype}")
    if int(stride) < 1:
        raise RuntimeError(f"{who}: stride must be >= 1, got {stride}")
    pairs = [tuple(int(v) for v in p) for p in pairs]
    if not pairs or any(len(p) != 2 for p in pairs):
        raise RuntimeError(f"{who}: pairs must be a non-empty list of (pred_id, gt_id)")
    pred = [points[labels == p][::stride] for p, _ in pairs]
    gt = [gt_points[gt_labels == g][::stride] for _, g in pairs]
    off1 = np.concatenate([[0], np.cumsum([t.shape[0] for t in pred])])
    off2 = np.concatenate([[0], np.cumsum([t.shape[0] for t in gt])])
    xyz1, xyz2 = torch.cat(pred).contiguous(), torch.cat(gt).contiguous()
    mean = chamfer_segments(xyz1, off1, xyz2, off2)[0]
    emd, residual = emd_segments(xyz1, off1, xyz2, off2, return_residual=True)
    host = torch.cat([_direction(who, mean, "bi")[:, None], emd[:, None], residual.double()], dim=1).cpu().numpy()
    out = []
    for b in range(len(pairs)):
        n1, n2 = int(off1[b + 1] - off1[b]), int(off2[b + 1] - off2[b])
        out.append(None if n1 == 0 or n2 == 0 else dict(n_pred=n1, n_gt=n2, cd=float(host[b, 0]), emd=float(host[b, 1]),
                                                        emd_residual=(float(host[b, 2]), float(host[b, 3]))))
    done = [r for r in out if r is not None]
    return out, dict(cd=sum(r["cd"] for r in done) / len(done) if done else None,
                     emd=sum(r["emd"] for r in done) / len(done) if done else None, evaluated=len(done))
