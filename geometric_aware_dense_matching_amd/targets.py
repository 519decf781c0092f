"""Ground-truth correspondence targets on the GPU: the reference loader's per-item geometry (get_pose_gt_info,
/root/reference/datasets/lm/linemod_pbr.py:602-655) for a whole batch, without leaving the device.

  visible_vertices   hidden-point removal (utils/compute_visibility.py:26-47 sphericalFlip + Qhull, :128-134 VisiblePoints)
  pose_gt_info       labels / match_idx / visible_flag / valid: the nearest visible posed vertex of every labelled point within 1 cm

Kernels: csrc/gdm_targets.hip (include/gdm.h gdm_hpr_visible_hip, gdm_pose_targets_hip).  No host synchronisation, so both
capture in a hipGraph.  The one deliberate deviation: by default the camera centre is fp32(-R^T t) evaluated in fp64, where the
reference inverts the fp32 4x4 pose with LAPACK (which can differ by an ulp, and the visibility is sensitive to it); pass
`cam_center` to use another centre.
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import call

HPR_PARAM = float(np.power(10.0, np.pi))            # compute_visibility.py:131 sphericalFlip(pts, c, math.pi)


def default_cam_center(RT):
    """The default camera centre of include/gdm.h, restated on the CPU (numpy): RT [B,3,4] -> f32[B,3] = fp32(-R^T t), the sums
    in fp64 as -((R_0k t_0 + R_1k t_1) + R_2k t_2)."""
    RT = np.asarray(RT, dtype=np.float32).reshape(-1, 3, 4).astype(np.float64)
    R, t = RT[:, :, :3], RT[:, :, 3]
    c = -((R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2]) + R[:, 2, :] * t[:, 2:3])
    return c.astype(np.float32)


def spherical_flip(model_xyz, center):
    """The flip of include/gdm.h restated on the CPU (numpy), bit-equal to the reference's sphericalFlip(model, center, pi) for
    f32 inputs: model f32[M,3], center f32[3] -> f64[M,3]."""
    p = np.asarray(model_xyz, dtype=np.float32) - np.asarray(center, dtype=np.float32).reshape(1, 3)
    n = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    rad = np.float64(n.max()) * HPR_PARAM
    n64 = n.astype(np.float64)[:, None]
    p64 = p.astype(np.float64)
    return (2.0 * ((rad - n64) * p64)) / n64 + p64


def _model_args(model_xyz, B):
    """model f32[M,3] (shared) or f32[B,M,3] -> (tensor, batch stride, M)."""
    m = ops._dev(model_xyz, torch.float32, "model_xyz")
    if m.dim() == 2 and m.shape[1] == 3:
        return m, 0, m.shape[0]
    if m.dim() == 3 and m.shape[0] == B and m.shape[2] == 3:
        return m, m.shape[1] * 3, m.shape[1]
    raise ValueError("model_xyz must be [M,3] or [B=%d,M,3], got %s" % (B, tuple(m.shape)))


def _cld_args(cld):
    """cld f32[B,N,3], or cld_rgb_nrm f32[B,C>=3,N] (rows 0-2 = xyz, as pose._scene_args) -> (tensor, bstride, pt, ch, N)."""
    c = ops._dev(cld, torch.float32, "cld")
    if c.dim() != 3:
        raise ValueError("cld must be [B,N,3] or cld_rgb_nrm [B,C,N], got %s" % (tuple(c.shape),))
    if c.shape[2] == 3 and c.shape[1] != 3:
        return c, c.stride(0), 3, 1, c.shape[1]
    if c.shape[1] >= 3 and c.shape[2] != 3:
        return c, c.stride(0), 1, c.shape[2], c.shape[2]
    raise ValueError("cld: ambiguous shape %s (pass [B,N,3] with N != 3 or [B,C,N] with N != 3)" % (tuple(c.shape),))


def _workspace(B, N, M, device):
    nbytes = int(_lib.lib().gdm_targets_workspace_bytes(B, N, M))
    if nbytes == 0:
        raise ValueError("targets: bad shape B=%d N=%d M=%d (M >= 4, B <= 65535)" % (B, N, M))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _hpr(model, mb, M, RT, cam_center, ws, nbytes):
    B = RT.shape[0]
    cam = None
    if cam_center is not None:
        cam = ops._dev(cam_center, torch.float32, "cam_center").reshape(B, 3).contiguous()
    flipped = torch.empty((B, M, 3), dtype=torch.float64, device=RT.device)
    visible = torch.empty((B, M), dtype=torch.uint8, device=RT.device)
    call("gdm_hpr_visible_hip", model, mb, RT, cam, B, M, ws, nbytes, flipped, visible)
    return visible, flipped


def _rt(RT):
    RT = ops._dev(RT, torch.float32, "RT")
    if RT.dim() != 3 or tuple(RT.shape[1:]) != (3, 4):
        raise ValueError("RT must be [B,3,4], got %s" % (tuple(RT.shape),))
    return RT


def visible_vertices(model_xyz, RT, cam_center=None, return_flipped=False):
    """Hidden-point removal of the model vertices seen from the camera of pose RT f32[B,3,4] (model -> camera, metres):
    model_xyz f32[M,3] or f32[B,M,3] -> visible u8[B,M] (the reference's VisiblePoints(model, inv_t.T) as a mask), and the flipped
    points f64[B,M,3] when return_flipped.  cam_center f32[B,3] overrides the default centre fp32(-R^T t)."""
    RT = _rt(RT)
    B = RT.shape[0]
    model, mb, M = _model_args(model_xyz, B)
    ws, nbytes = _workspace(B, 1, M, RT.device)
    visible, flipped = _hpr(model, mb, M, RT, cam_center, ws, nbytes)
    return (visible, flipped) if return_flipped else visible


def pose_gt_info(cld, labels, RT, model_xyz, dist_thresh=0.01, cam_center=None):
    """get_pose_gt_info (linemod_pbr.py:602-655) for a batch.  cld f32[B,N,3] or cld_rgb_nrm f32[B,C,N]; labels [B,N] (the mask at
    the chosen points, 255 already mapped to 1; any integer or bool dtype, > 0 = labelled); RT f32[B,3,4]; model_xyz f32[M,3]
    or f32[B,M,3] (metres).  -> dict(labels [B,N] (labels' dtype and values, 0 where a labelled point lost its match),
    match_idx i32[B,N] (M = no match), visible_flag u8[B,M], valid bool[B]).  Four kernels for the hidden-point removal plus three
    for the targets, no host synchronisation."""
    RT = _rt(RT)
    B = RT.shape[0]
    c, cb, ps, cs, N = _cld_args(cld)
    if c.shape[0] != B:
        raise ValueError("cld has %d crops, RT %d" % (c.shape[0], B))
    if not (float(dist_thresh) > 0.0):
        raise ValueError("dist_thresh=%r must be > 0" % (dist_thresh,))
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError("labels must be a CUDA (HIP) tensor: the geoMatch ops have no CPU fallback")
    if tuple(labels.shape) != (B, N):
        raise ValueError("labels must be [B=%d,N=%d], got %s" % (B, N, tuple(labels.shape)))
    lab = (labels > 0).to(torch.uint8).contiguous()                       # labelled = pt_labels > 0 (linemod_pbr.py:612, :624)
    model, mb, M = _model_args(model_xyz, B)
    ws, nbytes = _workspace(B, N, M, RT.device)
    visible, _ = _hpr(model, mb, M, RT, cam_center, ws, nbytes)
    labels_out = torch.empty((B, N), dtype=torch.uint8, device=RT.device)
    match_idx = torch.empty((B, N), dtype=torch.int32, device=RT.device)
    visible_flag = torch.empty((B, M), dtype=torch.uint8, device=RT.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=RT.device)
    call("gdm_pose_targets_hip", c, cb, ps, cs, lab, RT, model, mb, visible, B, N, M, float(dist_thresh), ws, nbytes, labels_out,
         match_idx, visible_flag, valid)
    # the kernels mark the labelled points that lost their label (filtered_pt_labels[...] = 0, :651); every other value is the input's
    lost = (lab != 0) & (labels_out == 0)
    labels_out = torch.where(lost, torch.zeros_like(labels), labels)
    return dict(labels=labels_out, match_idx=match_idx, visible_flag=visible_flag, valid=valid.bool())
