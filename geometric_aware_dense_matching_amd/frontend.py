"""GPU-side front end: from a device-resident RGB-D frame and a detection box to the model's input dict, so that the
DataLoader only ships the frame.  Mirrors the geometric part of the reference loader
(/root/reference/datasets/lm/linemod_pbr.py): depth -> xyz (`dpt_2_pcld` :398-411), the surface normals from the depth image
(:460-463), the padded / jittered detection box (`aug_bbox_DZI` :99-120), the S x S crop resampled around it (:468-473), valid-pixel
sampling of N points with wrap-around padding (:476-496), `cld_rgb_nrm` / `choose` assembly (:498-513) and the neighbour pyramid
(:515-569).

  make_inputs             integer S x S crops of a frame whose rgb is normalised and whose normals are given
  depth_normals           depth -> normal map (csrc/gdm_frontend.hip; the definition is in include/gdm.h)
  dzi_boxes               box -> centre and scale (torch, on the boxes' device; jitter="hash": one launch, counter-based draws)
  crop_from_boxes         the resampling crop: rgb, normals, dpt_xyz, depth, mask from one launch
  fill_depth              depth completion of the crop (csrc/gdm_depthfill.hip), the step the YCB-V item adds
  augment_crops           the YCB-V training item's colour / noise / background augmentation of the crop (csrc/gdm_augment.hip)
  make_inputs_from_boxes  raw uint8 rgb + depth + K + box (+ mask) -> the input dict, no host step and no host synchronisation;
                          depth_fill=None is the LineMOD item, "multiscale" / "fast" the YCB-V item
                          (/root/reference/datasets/ycbv/ycbv_pbr.py:458-509)
                          sampler="hash": the N points by the written rule of include/gdm.h and the assembly in one launch
                          (ops.sample_assemble, csrc/gdm_sample.hip) instead of sample_valid_pixels and the torch gathers

`depth_normals_numpy`, `crop_from_boxes_numpy`, `fill_depth_numpy`, `augment_crops_numpy`, `dzi_boxes_numpy` and
`sample_assemble_numpy` restate the kernels' definitions on the CPU (as
targets.spherical_flip does for the flip); the device results equal them value for value, up to the fp32 rounding of the bilateral
filter's exponentials in the last stage of the fill.  Parity with normalSpeed and with a given cv2 build is unpinned (DESIGN.md 6d,
6e)."""
import numpy as np
import torch

from . import _lib, ops, pyramid
from ._lib import call


def depth_to_xyz(depth, K, origin, S):
    """depth f32[B,H,W] (m), K f32[B,3,3], origin i32[B,2] = (x0,y0) -> xyz f32[B,S,S,3]."""
    depth = ops._dev(depth, torch.float32, "depth")
    K = ops._dev(K, torch.float32, "K")
    origin = ops._idx32(origin, "origin")
    B, H, W = depth.shape
    out = torch.empty((B, S, S, 3), dtype=torch.float32, device=depth.device)
    call("gdm_depth_to_xyz_hip", depth, K, origin, B, H, W, S, out)
    return out


def sample_valid_pixels(xyz, n_points, generator=None, valid=None):
    """Choose n_points valid pixels (z > 1e-6, or where `valid` bool[B,S,S] is set when it is given) per crop uniformly without
    replacement, in random order; crops with fewer valid pixels wrap around (np.pad(..., 'wrap'), linemod_pbr.py:492).
    xyz f32[B,S,S,3] -> choose i32[B,1,N]."""
    B, S = xyz.shape[0], xyz.shape[1]
    if valid is None:
        valid = xyz[..., 2].reshape(B, S * S) > 1e-6
    else:
        if valid.dtype != torch.bool or tuple(valid.shape) != (B, S, S):
            raise ValueError("valid must be bool[B=%d,S=%d,S=%d], got %s %s" % (B, S, S, valid.dtype, tuple(valid.shape)))
        valid = valid.reshape(B, S * S)
    key = torch.rand((B, S * S), device=xyz.device, generator=generator)
    key = torch.where(valid, key, key + 2.0)                       # invalid pixels sort last
    order = torch.argsort(key, dim=1)                              # random permutation of the valid pixels first
    nvalid = valid.sum(dim=1, keepdim=True).clamp(min=1)
    j = torch.arange(n_points, device=xyz.device).unsqueeze(0) % nvalid      # wrap-around padding
    return torch.gather(order, 1, j).to(torch.int32).unsqueeze(1)


def make_inputs(rgb_norm, depth, normals, K, origin, S, n_points, generator=None, mask=None):
    """rgb_norm f32[B,3,H,W] (already colour-normalised), depth f32[B,H,W], normals f32[B,3,H,W], K f32[B,3,3],
    origin i32[B,2] -> the model's input dict incl. the neighbour pyramid, all on the device.  With the object mask [B,H,W]
    (any dtype) the dict also holds origin_labels [B,N]: the mask at the chosen points, 255 mapped to 1 (linemod_pbr.py:470,
    :501-502), the labels targets.pose_gt_info takes."""
    B = depth.shape[0]
    xyz = depth_to_xyz(depth, K, origin, S)                                          # [B,S,S,3]
    ys = (origin[:, 1:2].long() + torch.arange(S, device=depth.device)[None]).clamp(0, depth.shape[1] - 1)
    xs = (origin[:, 0:1].long() + torch.arange(S, device=depth.device)[None]).clamp(0, depth.shape[2] - 1)
    bidx = torch.arange(B, device=depth.device)[:, None, None]
    rgb_c = rgb_norm[bidx, :, ys[:, :, None], xs[:, None, :]].permute(0, 3, 1, 2).contiguous()       # [B,3,S,S]
    nrm_c = normals[bidx, :, ys[:, :, None], xs[:, None, :]].permute(0, 3, 1, 2).contiguous()
    choose = sample_valid_pixels(xyz, n_points, generator)                           # [B,1,N]
    ch = choose[:, 0].long()
    cld = torch.gather(xyz.reshape(B, S * S, 3), 1, ch[:, :, None].expand(-1, -1, 3))
    rgb_pt = torch.gather(rgb_c.reshape(B, 3, S * S), 2, ch[:, None, :].expand(-1, 3, -1))
    nrm_pt = torch.gather(nrm_c.reshape(B, 3, S * S), 2, ch[:, None, :].expand(-1, 3, -1))
    inputs = dict(rgb=rgb_c, cld_rgb_nrm=torch.cat([cld.transpose(1, 2), rgb_pt, nrm_pt], dim=1).contiguous(), choose=choose,
                  dpt_xyz=xyz)
    if mask is not None:
        msk = mask[bidx, ys[:, :, None], xs[:, None, :]].reshape(B, S * S)                  # [B,S*S], the crop of the mask
        lab = torch.gather(msk, 1, ch)
        inputs["origin_labels"] = torch.where(lab == 255, torch.ones_like(lab), lab)
    inputs.update(pyramid.build_pyramid(cld.contiguous(), xyz))
    return inputs


# --------------------------------------------------------------------------------------
# detection boxes: normals from depth, the resampling crop, the whole item
# --------------------------------------------------------------------------------------
COLOR_MEAN = (0.485, 0.456, 0.406)                  # normalize_color (/root/reference/utils/ply.py:502-509), as csrc/gdm_frontend.hip
COLOR_STD_CROP = (0.229, 0.224, 0.224)
NORMALS_MAX_K = _lib.GDM_NORMALS_MAX_K


def _depth_mm(depth):
    """(uint16) trunc(fp32(depth) * 1000.0f) as int64; negative and NaN -> 0, 65.535 m and beyond -> 65535."""
    v = np.asarray(depth, dtype=np.float32) * np.float32(1000.0)
    with np.errstate(invalid="ignore"):
        return np.where(v >= 65535.0, 65535.0, np.where(v >= 0.0, np.trunc(v), 0.0)).astype(np.int64)


def depth_normals_numpy(depth, K, k_size=5, distance_threshold=2000, difference_threshold=20):
    """The definition of `depth_normals` (include/gdm.h gdm_depth_normals_hip) restated on the CPU: depth f32[B,H,W] (m),
    K f32[B,3,3] -> normals f32[B,3,H,W]."""
    depth = np.asarray(depth, dtype=np.float32)
    K = np.asarray(K, dtype=np.float32)
    B, H, W = depth.shape
    r = int(k_size)
    d = _depth_mm(depth)
    out = np.zeros((B, 3, H, W), np.float32)
    if H <= 2 * r or W <= 2 * r:
        return out
    c = d[:, r:H - r, r:W - r]
    A0, A1, A3, b0, b1 = (np.zeros(c.shape, np.int64) for _ in range(5))
    for j in (-r, 0, r):
        for i in (-r, 0, r):
            if i == 0 and j == 0:
                continue
            delta = d[:, r + j:H - r + j, r + i:W - r + i] - c
            f = (np.abs(delta) < int(difference_threshold)).astype(np.int64)
            A0 += f * (i * i)
            A1 += f * (i * j)
            A3 += f * (j * j)
            b0 += f * i * delta
            b1 += f * j * delta
    det = A0 * A3 - A1 * A1
    ddx = A3 * b0 - A1 * b1
    ddy = -A1 * b0 + A0 * b1
    nx = K[:, 0, 0][:, None, None] * ddx.astype(np.float32)
    ny = K[:, 1, 1][:, None, None] * ddy.astype(np.float32)
    nz = (-(det * c)).astype(np.float32)
    s = np.sqrt((nx * nx + ny * ny) + nz * nz)
    ok = (s > 0) & (c < int(distance_threshold))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.stack([nx / s, ny / s, nz / s], axis=1)
    out[:, :, r:H - r, r:W - r] = np.where(ok[:, None], n, np.float32(0.0))
    return out


def _fix10(v):
    """round-half-even(v * 1024) as int64 (v float64); NaN and anything beyond +-1e15 land on +-1e15."""
    with np.errstate(invalid="ignore"):
        w = np.asarray(v, dtype=np.float64) * 1024.0
        w = np.where(w > -1e15, w, -1e15)                          # NaN -> -1e15, as fmax(NaN, -1e15) on the device
        return np.rint(np.minimum(w, 1e15)).astype(np.int64)


def crop_from_boxes_numpy(rgb_u8, depth, normals, K, center, scale, S, mask=None):
    """The definition of `crop_from_boxes` (include/gdm.h gdm_warp_crop_hip) restated on the CPU, numpy arrays in and out:
    -> dict(rgb f32[B,3,S,S], normals f32[B,3,S,S], dpt_xyz f32[B,S,S,3], depth f32[B,S,S], mask u8[B,S,S] with a mask)."""
    rgb_u8 = np.asarray(rgb_u8, dtype=np.uint8)
    depth = np.asarray(depth, dtype=np.float32)
    normals = np.asarray(normals, dtype=np.float32)
    K = np.asarray(K, dtype=np.float32)
    center = np.asarray(center, dtype=np.float32).astype(np.float64)
    scale = np.asarray(scale, dtype=np.float32).astype(np.float64)
    B, H, W = depth.shape
    f32 = np.float32
    out = dict(rgb=np.zeros((B, 3, S, S), f32), normals=np.zeros((B, 3, S, S), f32), dpt_xyz=np.zeros((B, S, S, 3), f32),
               depth=np.zeros((B, S, S), f32))
    if mask is not None:
        mask = np.asarray(mask, dtype=np.uint8)
        out["mask"] = np.zeros((B, S, S), np.uint8)
    g = np.arange(S, dtype=np.float64)
    mean, std = np.array(COLOR_MEAN, f32), np.array(COLOR_STD_CROP, f32)
    for b in range(B):
        a = scale[b] / float(S)
        half = (a * float(S)) / 2.0
        bx, by = center[b, 0] - half, center[b, 1] - half
        rx = (_fix10(a * g) + _fix10(bx))[None, :]                 # [1,S]
        ry = _fix10(a * g + by)[:, None]                           # [S,1]
        X, Y = np.broadcast_arrays((rx + 512) >> 10, (ry + 512) >> 10)
        X5, Y5 = (rx + 16) >> 5, (ry + 16) >> 5
        sx, al, sy, be = X5 >> 5, X5 & 31, Y5 >> 5, Y5 & 31

        def taps(img):                                             # img [H,W,...] -> the four taps, 0 outside the frame
            res = []
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                yy, xx = np.broadcast_arrays(sy + dy, sx + dx)
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
                res.append(np.where(ok.reshape(ok.shape + (1,) * (v.ndim - 2)), v, 0))
            return res

        wi = [32 * (32 - be) * (32 - al), 32 * (32 - be) * al, 32 * be * (32 - al), 32 * be * al]
        t = taps(rgb_u8[b].astype(np.int64))
        acc = sum(w[..., None] * v for w, v in zip(wi, t))
        c = ((acc + 16384) >> 15).astype(f32) / f32(255.0)
        c = c - mean
        c = c / std
        out["rgb"][b] = c.transpose(2, 0, 1)
        fb, fa = be.astype(f32) / f32(32.0), al.astype(f32) / f32(32.0)
        one = f32(1.0)
        wf = [((one - fb) * (one - fa))[..., None], ((one - fb) * fa)[..., None], (fb * (one - fa))[..., None], (fb * fa)[..., None]]
        t = [v.astype(f32) for v in taps(normals[b].transpose(1, 2, 0))]
        n = ((t[0] * wf[0] + t[1] * wf[1]) + t[2] * wf[2]) + t[3] * wf[3]
        out["normals"][b] = n.transpose(2, 0, 1)
        ok = (Y >= 0) & (Y < H) & (X >= 0) & (X < W)
        Yc, Xc = np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)
        d = np.where(ok, depth[b][Yc, Xc], f32(0.0)).astype(f32)
        out["depth"][b] = d
        if mask is not None:
            out["mask"][b] = np.where(ok, mask[b][Yc, Xc], 0)
        d64 = d.astype(np.float64)
        m = (d > f32(1e-8)).astype(np.float64)
        k = K[b].astype(np.float64)
        out["dpt_xyz"][b] = np.stack([(X.astype(np.float64) - k[0, 2]) * d64 / k[0, 0] * m,
                                      (Y.astype(np.float64) - k[1, 2]) * d64 / k[1, 1] * m, d64 * m], axis=2).astype(f32)
    return out


# the structuring elements of depth completion (include/gdm.h gdm_fill_depth_hip), as (dy, dx) tap lists
def _full(n):
    r = n // 2
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def _cross(n):
    r = n // 2
    return [(dy, dx) for dy, dx in _full(n) if dy == 0 or dx == 0]


_DIAMOND_5 = [(dy, dx) for dy, dx in _full(5) if abs(dy) + abs(dx) <= 2]
FILL_MODES = {"multiscale": _lib.GDM_FILL_MULTISCALE, "fast": _lib.GDM_FILL_FAST}
FILL_STAGES = _lib.GDM_FILL_STAGES
_FILL_STAGE_NAMES = ("s1_inverted_depths", "s2_dilated_depths", "s3_closed_depths", "s4_blurred_depths", "s5_combined_depths",
                     "s7_before_bilateral", "s7_blurred_depths")


def _morph(a, taps, op):
    """max (op = np.maximum) or min over the taps; a tap outside the image is ignored.  a f32[B,H,W]."""
    B, H, W = a.shape
    r = max(max(abs(dy), abs(dx)) for dy, dx in taps)
    pad = np.pad(a, ((0, 0), (r, r), (r, r)), constant_values=-np.inf if op is np.maximum else np.inf)
    out = a.copy()
    for dy, dx in taps:
        out = op(out, pad[:, r + dy:r + dy + H, r + dx:r + dx + W])
    return out


def _median5(a):
    """The 13th smallest of the 5 x 5 window, replicated border."""
    B, H, W = a.shape
    pad = np.pad(a, ((0, 0), (2, 2), (2, 2)), mode="edge")
    win = np.stack([pad[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W] for dy, dx in _full(5)], axis=0)
    return np.sort(win, axis=0)[12]


def _reflect101(n):
    """Source index of positions -2 .. n+1: reflected (-1 -> 1, n -> n-2), then clamped to the image."""
    p = np.abs(np.arange(-2, n + 2))
    p = np.where(p >= n, 2 * n - 2 - p, p)
    return np.clip(p, 0, n - 1)


def _bilateral(a, sigma_color, sigma_space):
    """The bilateral filter of the definition: 13 taps in row-major order, fp32, one rounding per operation."""
    f32 = np.float32
    B, H, W = a.shape
    pad = a[:, _reflect101(H)[:, None], _reflect101(W)[None, :]]
    cc = f32(-0.5 / (sigma_color * sigma_color))
    g = -0.5 / (sigma_space * sigma_space)
    num, den = np.zeros_like(a), np.zeros_like(a)
    with np.errstate(over="ignore", invalid="ignore"):
        for dy, dx in _full(5):
            r2 = dx * dx + dy * dy
            if r2 > 4:
                continue
            v = pad[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
            dv = v - a
            e = (dv * dv) * cc
            w = f32(np.exp(float(r2) * g)) * np.exp(e)
            num = num + w * v
            den = den + w
        return num / den


def _column_top_mask(valid):
    """top[y,x] = y >= the first valid row of column x; a column without one has first row 0 (np.argmax of all-False)."""
    H = valid.shape[1]
    return np.arange(H)[None, :, None] >= np.argmax(valid, axis=1)[:, None, :]


def fill_depth_numpy(depth, mode="multiscale", max_depth=100.0, return_stages=False, extrapolate=False, blur_type="bilateral"):
    """The definition of `fill_depth` (include/gdm.h gdm_fill_depth_hip) restated on the CPU: depth f32[B,H,W] (m) -> f32[B,H,W],
    IP-Basic's fill_in_multiscale / fill_in_fast with the defaults the YCB-V loader uses (/root/reference/utils/ip_basic/
    depth_map_utils.py:133-286, :66-130).  With return_stages also a dict of the intermediate images under the reference's
    process_dict names (s1_inverted_depths ... s8_inverted_depths; s6_extended_depths is s5_combined_depths without extrapolation)
    plus s7_before_bilateral, the image the bilateral filter reads; the fast mode has no s4 and no s6."""
    if mode not in FILL_MODES:
        raise ValueError("mode must be 'multiscale' or 'fast', got %r" % (mode,))
    if extrapolate or blur_type != "bilateral":
        raise ValueError("only extrapolate=False and blur_type='bilateral' are defined (the loader passes nothing else)")
    f32 = np.float32
    d = np.asarray(depth, dtype=f32)
    if d.ndim != 3:
        raise ValueError("depth must be [B,H,W], got %s" % (d.shape,))
    with np.errstate(invalid="ignore"):
        d = np.where(d > 0, d, f32(0.0))
    md, t = f32(max_depth), f32(0.1)

    def inv(a):
        return np.where(a > t, md - a, a)

    st = {}
    s1 = inv(d)
    if mode == "multiscale":
        near, med, far = (d > t) & (d <= f32(15.0)), (d > f32(15.0)) & (d <= f32(30.0)), d > f32(30.0)
        s2 = s1
        for sel, taps in ((far, _cross(3)), (med, _cross(5)), (near, _cross(7))):
            dil = _morph(np.where(sel, s1, f32(0.0)), taps, np.maximum)
            s2 = np.where(dil > t, dil, s2)
        s3 = _morph(_morph(s2, _full(5), np.maximum), _full(5), np.minimum)
        s4 = np.where(s3 > t, _median5(s3), s3)
        s5 = np.where(~(s4 > t) & _column_top_mask(s4 > t), _morph(s4, _full(9), np.maximum), s4)
        top = _column_top_mask(s5 > t)
        s7 = s5
        for _ in range(6):
            s7 = np.where((s7 < t) & top, _morph(s7, _full(5), np.maximum), s7)
        valid = (s7 > t) & top
        m = np.where(valid, _median5(s7), s7)
        f = np.where(valid, _bilateral(m, 0.5, 2.0), m)
        st.update(s4_blurred_depths=s4, s6_extended_depths=s5)
    else:
        s2 = _morph(s1, _DIAMOND_5, np.maximum)
        s3 = _morph(_morph(s2, _full(5), np.maximum), _full(5), np.minimum)
        s5 = np.where(s3 < t, _morph(s3, _full(7), np.maximum), s3)
        m = _median5(s5)
        f = _bilateral(m, 1.5, 2.0)
    out = inv(f).astype(f32)
    if not return_stages:
        return out
    st.update(s1_inverted_depths=s1, s2_dilated_depths=s2, s3_closed_depths=s3, s5_combined_depths=s5, s7_before_bilateral=m,
              s7_blurred_depths=f, s8_inverted_depths=out)
    return out, {k: st[k] for k in sorted(st)}


def _mix32(x):
    """lowbias32 on uint32 arrays (include/gdm.h; the same function as pose._mix32)."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def sample_keys(B, P, seed=0):
    """key(p) of include/gdm.h gdm_sample_assemble_hip for every crop and pixel: u32[B,P]."""
    with np.errstate(over="ignore"):
        hb = _mix32(_mix32(np.uint32(int(seed) & 0xffffffff) ^ np.uint32(0x9e3779b9)) ^ np.arange(B, dtype=np.uint32))
        return _mix32(hb[:, None] ^ np.arange(P, dtype=np.uint32)[None, :])


def sample_assemble_numpy(valid_depth, dpt_xyz, rgb, normals, mask, N, seed=0):
    """The definition of `ops.sample_assemble` (include/gdm.h gdm_sample_assemble_hip) restated on the CPU: valid_depth f32[B,S,S]
    (or [B,P]), dpt_xyz f32[B,S,S,3], rgb f32[B,3,S,S], normals f32[B,3,S,S], mask u8[B,S,S] or None -> choose i32[B,N],
    cld_rgb_nrm f32[B,9,N], labels u8[B,N] (None without a mask), n_valid i32[B]."""
    vd = np.asarray(valid_depth, dtype=np.float32)
    B = vd.shape[0]
    vd = vd.reshape(B, -1)
    P = vd.shape[1]
    xyz = np.asarray(dpt_xyz, dtype=np.float32).reshape(B, P, 3)
    rgb = np.asarray(rgb, dtype=np.float32).reshape(B, 3, P)
    nrm = np.asarray(normals, dtype=np.float32).reshape(B, 3, P)
    with np.errstate(invalid="ignore"):
        valid = vd > np.float32(1e-6)                              # NaN and negative depth compare false
    keys = sample_keys(B, P, seed)
    choose = np.zeros((B, N), np.int32)
    n_valid = valid.sum(axis=1).astype(np.int32)
    for b in range(B):
        pix = np.nonzero(valid[b])[0]
        if pix.size:
            order = pix[np.argsort(keys[b, pix], kind="stable")]   # the keys of a crop are distinct: no tie to break
            choose[b] = order[np.arange(N) % pix.size]
    ch3 = np.repeat(choose[:, None, :], 3, axis=1).astype(np.int64)                    # [B,3,N]
    cld_rgb_nrm = np.concatenate([np.take_along_axis(xyz.transpose(0, 2, 1), ch3, axis=2), np.take_along_axis(rgb, ch3, axis=2),
                                  np.take_along_axis(nrm, ch3, axis=2)], axis=1).astype(np.float32)
    labels = None
    if mask is not None:
        lab = np.take_along_axis(np.asarray(mask, dtype=np.uint8).reshape(B, P), choose.astype(np.int64), axis=1)
        labels = np.where(lab == 255, np.uint8(1), lab).astype(np.uint8)
    return choose, cld_rgb_nrm, labels, n_valid


# --------------------------------------------------------------------------------------
# the YCB-V training item's augmentation of the crop (include/gdm.h gdm_augment_crops_hip)
# --------------------------------------------------------------------------------------
AUG_C = 0x85ebca6b                                             # the constant of the augmentation's draws (the sampler's is 0x9e3779b9)
DZI_C = 0xc2b2ae35                                             # the constant of the hash-drawn box jitter
AUG_MIN_S = _lib.GDM_AUG_MIN_S
_P20, _P80 = 0xcccccccc, 0x33333333                            # word > _P20: probability 0.2; word > _P80: probability 0.8
_aug_tab = {}


def aug_tables():
    """The integer tables of csrc/gdm_augment_tables.h (tools/make_aug_tables.py writes them): gdm_aug_cos_q14 [360],
    gdm_aug_gauss3 [256,2], gdm_aug_gauss5 [256,3], read from the header the kernel is compiled with."""
    if not _aug_tab:
        import os
        import re
        txt = open(os.path.join(_lib.CSRC, "gdm_augment_tables.h")).read()
        for name, dims, body in re.findall(r"GDM_AUG_TABLE short (\w+)((?:\[\d+\])+) = \{(.*?)\};", txt, flags=re.S):
            shape = [int(d) for d in re.findall(r"\d+", dims)]
            _aug_tab[name] = np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int64).reshape(shape)
    return _aug_tab


def _mix1(x):
    """lowbias32 on one Python int."""
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    return x ^ (x >> 16)


def _below(w, n):
    return (w * n) >> 32


def motion_taps(angle, length):
    """The taps of linear_motion_blur's a x a kernel by the written rule: (a, [(dy, dx), ...]); a <= 0 -> (a, None), the image as it is."""
    cos = aug_tables()["gdm_aug_cos_q14"]
    cs, sn = int(cos[angle % 360]), int(cos[(angle + 270) % 360])
    a = (max(abs(cs), abs(sn)) * length * 2) >> 14
    if a <= 0:
        return a, None

    def trunc(v):
        return v // 16384 if v >= 0 else -((-v) // 16384)

    cx = a // 2
    ex, ey = cx + trunc(cs * length), cx + trunc(sn * length)
    dx, sx = abs(ex - cx), (1 if ex > cx else -1)
    dy, sy = -abs(ey - cx), (1 if ey > cx else -1)
    err, x, y, taps = dx + dy, cx, cx, []
    while True:
        if 0 <= x < a and 0 <= y < a:
            taps.append((y - cx, x - cx))
        if x == ex and y == ey:
            break
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy
    return a, taps


def _draw_pass(hb, q):
    D = lambda j: _mix1(hb ^ (16 * q + j))                     # noqa: E731
    t = aug_tables()
    p = dict(ks=320 + _below(D(0), 52), kv=294 + _below(D(1), 52), sharpen=D(2) > _P20, sharpen_u=D(3) >> 24, motion=D(4) > _P20,
             angle=_below(D(5), 360), length=_below(D(6), 15) + 1, gauss=D(7) > _P20, gauss_k=3 if D(8) > _P80 else 5,
             gauss_level=D(9) >> 24, sigma=_below(D(11), 15 if D(10) > _P80 else 25), extra=D(12) > _P20,
             hs=(_mix1(hb ^ (256 + 2 * q)), _mix1(hb ^ (256 + 2 * q + 1))))
    p["a"], p["taps"] = motion_taps(p["angle"], p["length"])
    p["gauss_w"] = [int(v) for v in (t["gdm_aug_gauss3"] if p["gauss_k"] == 3 else t["gdm_aug_gauss5"])[p["gauss_level"]]]
    reach_m = max(max(abs(dy), abs(dx)) for dy, dx in p["taps"]) if p["motion"] and p["taps"] else 0
    p["halo"] = (1 if p["sharpen"] else 0) + reach_m + (p["gauss_k"] // 2 if p["gauss"] else 0)
    return p


def augment_draws_numpy(B, seed, S=None, bank_shape=None):
    """Every per-crop decision of `augment_crops` for crops 0 .. B-1 and an int seed, as a list of dicts: passes = [pass 0, pass 1], each
    with the gains ks, kv (1/256), sharpen / sharpen_u, motion / angle / length / a (the kernel's side) / taps [(dy, dx)], gauss /
    gauss_k / gauss_level / gauss_w, sigma, extra, halo (the pixels a tile of that pass reads beyond itself) and the hashes hs of its
    two noise streams; second: whether pass 1 is applied; bank_words: the three words of the paste, and with S and
    bank_shape = (Nb, Hb, Wb) also bank, wy, wx."""
    out = []
    for b in range(B):
        hb = _mix1(_mix1((int(seed) & 0xffffffff) ^ AUG_C) ^ b)
        d = dict(hb=hb, passes=[_draw_pass(hb, 0), _draw_pass(hb, 1)], second=_mix1(hb ^ 32) > _P20,
                 bank_words=(_mix1(hb ^ 33), _mix1(hb ^ 34), _mix1(hb ^ 35)))
        if bank_shape is not None:
            Nb, Hb, Wb = bank_shape
            w = d["bank_words"]
            d.update(bank=w[0] % Nb, wy=w[1] % (Hb - S - 1), wx=w[2] % (Wb - S - 1))
        out.append(d)
    return out


def aug_levels(x):
    """The uint8 levels of a normalised crop x f32[...,3,S,S] (include/gdm.h): int64, NaN -> 0."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    mean, std = np.array(COLOR_MEAN, f32).reshape(3, 1, 1), np.array(COLOR_STD_CROP, f32).reshape(3, 1, 1)
    with np.errstate(invalid="ignore"):
        f = ((x * std) + mean) * f32(255.0)
        f = np.where(f > 0, f, f32(0.0))
        return np.rint(np.minimum(f, f32(255.0))).astype(np.int64)


def aug_normalise(v):
    """normalize_color as csrc/gdm_frontend.hip does it: levels int[...,3,S,S] -> f32."""
    f32 = np.float32
    mean, std = np.array(COLOR_MEAN, f32).reshape(3, 1, 1), np.array(COLOR_STD_CROP, f32).reshape(3, 1, 1)
    c = np.asarray(v).astype(f32) / f32(255.0)
    c = c - mean
    return (c / std).astype(f32)


def _pad101(img, r):
    """img [H,W,...] extended by r pixels a side, BORDER_REFLECT_101."""
    def idx(n):
        i = np.abs(np.arange(-r, n + r))
        return np.where(i >= n, 2 * n - 2 - i, i)
    return img[idx(img.shape[0])[:, None], idx(img.shape[1])[None, :]]


def aug_hsv_gain(img, ks, kv):
    """Step 1: img int64[H,W,3] -> int64[H,W,3]."""
    M, m = img.max(axis=2), img.min(axis=2)
    d = M - m
    M2 = np.minimum(255, (M * kv) >> 8)
    s = np.where(M > 0, (255 * d + (M >> 1)) // np.maximum(M, 1), 0)
    s2 = np.minimum(255, (s * ks) >> 8)
    m2 = M2 - (M2 * s2 + 127) // 255
    out = m2[..., None] + ((img - m[..., None]) * (M2 - m2)[..., None] + (d >> 1)[..., None]) // np.maximum(d, 1)[..., None]
    return np.where((d > 0)[..., None], out, M2[..., None])


def aug_sharpen(img, u):
    H, W = img.shape[:2]
    pad = _pad101(img, 1)
    s8 = sum(pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
    c256, q = 2304 + 3 * u, 256 + 3 * u
    return np.clip((2 * (c256 * img - 256 * s8) + q) // (2 * q), 0, 255)


def aug_motion(img, taps):
    if not taps:
        return img
    H, W = img.shape[:2]
    r = max(max(abs(dy), abs(dx)) for dy, dx in taps)
    pad = _pad101(img, r)
    n = len(taps)
    return (sum(pad[r + dy:r + dy + H, r + dx:r + dx + W] for dy, dx in taps) + (n >> 1)) // n


def aug_gauss(img, w):
    H, W = img.shape[:2]
    r = len(w) - 1
    pad = _pad101(img, r)
    acc = sum(w[abs(dy)] * w[abs(dx)] * pad[r + dy:r + dy + H, r + dx:r + dx + W] for dy in range(-r, r + 1) for dx in range(-r, r + 1))
    return (acc + 32768) >> 16


def aug_noise(img, sigma, hs):
    """v + ((z sigma 443 + 32768) >> 16), clipped; the word of pixel p = y W + x (a square image: W = S), channel c is mix(hs ^ (3 p + c))."""
    H, W = img.shape[:2]
    with np.errstate(over="ignore"):
        w = _mix32(np.uint32(hs) ^ np.arange(3 * H * W, dtype=np.uint32)).reshape(H, W, 3).astype(np.int64)
    z = (w & 255) + ((w >> 8) & 255) + ((w >> 16) & 255) + (w >> 24) - 510
    return np.clip(img + ((z * sigma * 443 + 32768) >> 16), 0, 255)


def aug_pass(img, p):
    """One pass of rgb_add_noise with the draws p (an entry of augment_draws_numpy's passes): img int64[S,S,3] -> int64[S,S,3]."""
    img = aug_hsv_gain(img, p["ks"], p["kv"])
    if p["sharpen"]:
        img = aug_sharpen(img, p["sharpen_u"])
    if p["motion"]:
        img = aug_motion(img, p["taps"])
    if p["gauss"]:
        img = aug_gauss(img, p["gauss_w"])
    img = aug_noise(img, p["sigma"], p["hs"][0])
    if p["extra"]:
        img = aug_noise(img, 7, p["hs"][1])
    return img


def aug_paste(img, depth, mask, bg_rgb, bg_depth, bg_mask, n, wy, wx):
    """add_real_back on one crop: img int[S,S,3], depth f32[S,S], mask u8[S,S] and the S x S window at (wy, wx) of the bank's frame n ->
    (img, depth): the object's pixels (mask > 0) and the valid depths (> 1e-6) stay, the rest is the window where bg_mask < 255, else 0."""
    S = depth.shape[0]
    ys, xs = slice(wy, wy + S), slice(wx, wx + S)
    keep = bg_mask[n, ys, xs] < 255
    back = np.where(keep[..., None], bg_rgb[n, ys, xs].astype(np.int64), 0)
    with np.errstate(invalid="ignore"):
        d = np.where(depth > np.float32(1e-6), depth, np.where(keep, bg_depth[n, ys, xs], np.float32(0.0))).astype(np.float32)
    return np.where((mask > 0)[..., None], img, back), d


def augment_crops_numpy(rgb, depth, mask=None, background=None, enable=None, seed=0):
    """The definition of `augment_crops` (include/gdm.h gdm_augment_crops_hip) restated on the CPU, numpy arrays in and out:
    rgb f32[B,3,S,S], depth f32[B,S,S], mask u8[B,S,S], background = (bg_rgb u8[Nb,Hb,Wb,3], bg_depth f32[Nb,Hb,Wb], bg_mask
    u8[Nb,Hb,Wb]) or None, enable u8[B] or None, an int seed -> (rgb f32[B,3,S,S], depth f32[B,S,S])."""
    rgb = np.asarray(rgb, dtype=np.float32)
    depth = np.asarray(depth, dtype=np.float32)
    B, S = depth.shape[0], depth.shape[1]
    if rgb.shape != (B, 3, S, S) or depth.shape != (B, S, S):
        raise ValueError("rgb must be [B,3,S,S] and depth [B,S,S], got %s and %s" % (rgb.shape, depth.shape))
    if S < AUG_MIN_S:
        raise ValueError("S=%d is below %d (a blur reaches 15 pixels)" % (S, AUG_MIN_S))
    bank_shape = None
    if background is not None:
        if mask is None:
            raise ValueError("the background paste needs the crop's mask")
        bg_rgb, bg_depth, bg_mask = (np.asarray(background[0], np.uint8), np.asarray(background[1], np.float32),
                                     np.asarray(background[2], np.uint8))
        bank_shape = bg_rgb.shape[:3]
        if bank_shape[1] < S + 2 or bank_shape[2] < S + 2:
            raise ValueError("the bank's frames must be at least S + 2 a side")
    draws = augment_draws_numpy(B, seed, S, bank_shape)
    out_rgb, out_depth = rgb.copy(), depth.copy()
    for b, d in enumerate(draws):
        if enable is not None and not np.asarray(enable)[b]:
            continue
        img = aug_pass(aug_levels(rgb[b]).transpose(1, 2, 0), d["passes"][0])
        if background is not None:
            img, out_depth[b] = aug_paste(img, depth[b], np.asarray(mask)[b], bg_rgb, bg_depth, bg_mask, d["bank"], d["wy"], d["wx"])
        if d["second"]:
            img = aug_pass(img, d["passes"][1])
        out_rgb[b] = aug_normalise(img.transpose(2, 0, 1))
    return out_rgb, out_depth


def augment_crops(rgb, depth, mask=None, background=None, enable=None, seed=0):
    """`ops.augment_crops`: the augmentation of the YCB-V training crop on the device (ycbv_pbr.py:468-477), the definition
    `augment_crops_numpy` restates -> (rgb, depth).  `augment_draws_numpy(B, seed)` tells what an int seed applies to every crop."""
    return ops.augment_crops(rgb, depth, mask=mask, background=background, enable=enable, seed=seed)


_fill_workspace = {}                                           # device -> the grow-only workspace of fill_depth


def fill_depth(depth, mode="multiscale", max_depth=100.0, return_stages=False, extrapolate=False, blur_type="bilateral"):
    """Depth completion of cropped depth images, the YCB-V loader's `fill_missing(dpt, 1, 1)` (ycbv_pbr.py:477): depth f32[B,H,W]
    (m, any H, W >= 1) -> f32[B,H,W], the definition `fill_depth_numpy` restates.  mode "multiscale" (a memset and three launches) or
    "fast" (one launch), whatever B.  With return_stages also the dict of intermediate images `fill_depth_numpy` returns."""
    if mode not in FILL_MODES:
        raise ValueError("mode must be 'multiscale' or 'fast', got %r" % (mode,))
    if extrapolate or blur_type != "bilateral":
        raise ValueError("only extrapolate=False and blur_type='bilateral' are defined (the loader passes nothing else)")
    depth = ops._dev(depth, torch.float32, "depth")
    if depth.dim() != 3:
        raise ValueError("depth must be [B,H,W], got %s" % (tuple(depth.shape),))
    B, H, W = depth.shape
    lib, m = _lib.lib(), FILL_MODES[mode]
    need = lib.gdm_fill_depth_workspace_bytes(B, H, W, m)
    if need and ops._pool is not ops._default_pool:                # inside a BufferPool scope (a captured step): the owner's scratch buffer,
        ws = ops._workspace(need, depth.device)                    # which no later, larger call can replace under the graph
    else:
        ws = _fill_workspace.get(depth.device)
        if need and (ws is None or ws.numel() < need):
            ws = _fill_workspace[depth.device] = torch.empty(need, dtype=torch.uint8, device=depth.device)
    out = torch.empty_like(depth)
    stages = torch.empty((FILL_STAGES, B, H, W), dtype=torch.float32, device=depth.device) if return_stages else None
    call("gdm_fill_depth_hip", depth, B, H, W, m, float(max_depth), ws if need else None, ws.numel() if need else 0, out, stages)
    if not return_stages:
        return out
    st = {name: stages[i] for i, name in enumerate(_FILL_STAGE_NAMES) if not (mode == "fast" and i == 3)}
    if mode == "multiscale":
        st["s6_extended_depths"] = st["s5_combined_depths"]
    st["s8_inverted_depths"] = out
    return out, {k: st[k] for k in sorted(st)}


def depth_normals(depth, K, k_size=5, distance_threshold=2000, difference_threshold=20):
    """Surface normals from the depth image, the loader's normalSpeed.depth_normal(dpt_mm, fx, fy, 5, 2000, 20, False)
    (linemod_pbr.py:460-463): depth f32[B,H,W] (m), K f32[B,3,3] -> normals f32[B,3,H,W], unit vectors towards the camera
    (nz <= 0), zero on the k_size border, beyond distance_threshold (mm) and where no gradient can be fitted.  One launch."""
    depth = ops._dev(depth, torch.float32, "depth")
    K = ops._dev(K, torch.float32, "K")
    if depth.dim() != 3 or tuple(K.shape) != (depth.shape[0], 3, 3):
        raise ValueError("depth must be [B,H,W] and K [B,3,3], got %s and %s" % (tuple(depth.shape), tuple(K.shape)))
    B, H, W = depth.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=depth.device)
    call("gdm_depth_normals_hip", depth, K, B, H, W, int(k_size), int(distance_threshold), int(difference_threshold), out)
    return out


def _dzi_torch(box, im_hw, pad_ratio, scale_ratio, shift_ratio, u):
    """The arithmetic of `dzi_boxes` on box f32[B,4] and the draws u f32[B,3] in [-1, 1) (None: no jitter)."""
    x1, y1, x2, y2 = box.unbind(1)
    bw, bh = x2 - x1, y2 - y1
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    if u is not None:
        cx = cx + bw * (shift_ratio * u[:, 1])
        cy = cy + bh * (shift_ratio * u[:, 2])
        scale = torch.maximum(bh, bw) * (1.0 + scale_ratio * u[:, 0]) * pad_ratio
    else:
        scale = torch.maximum(bh, bw) * pad_ratio
    scale = scale.clamp(max=float(max(im_hw)))
    return torch.stack([cx, cy], dim=1), scale


def dzi_draws_numpy(B, seed):
    """The three U(-1,1) of every box under jitter="hash" (include/gdm.h gdm_dzi_boxes_hip): f32[B,3], each 2 (w >> 8) 2^-24 - 1."""
    with np.errstate(over="ignore"):
        hb = _mix32(_mix32(np.uint32(int(seed) & 0xffffffff) ^ np.uint32(DZI_C)) ^ np.arange(B, dtype=np.uint32))
        w = _mix32(hb[:, None] ^ np.arange(3, dtype=np.uint32)[None, :])
    return np.float32(2.0) * ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)) - np.float32(1.0)


def dzi_boxes_numpy(bbox_xyxy, im_hw, pad_ratio=1.5, scale_ratio=0.25, shift_ratio=0.25, train=False, seed=0, u=None):
    """The definition of `dzi_boxes(jitter="hash")` (include/gdm.h gdm_dzi_boxes_hip) restated on the CPU in fp32, one rounding per
    operation: bbox f32[B,4] -> center f32[B,2], scale f32[B].  `u` f32[B,3] replaces the hash draws of `seed` (to compare with the
    torch arithmetic on given numbers)."""
    f32 = np.float32
    box = np.asarray(bbox_xyxy, dtype=f32)
    x1, y1, x2, y2 = box[:, 0], box[:, 1], box[:, 2], box[:, 3]
    bw, bh = x2 - x1, y2 - y1
    cx, cy = f32(0.5) * (x1 + x2), f32(0.5) * (y1 + y2)
    with np.errstate(invalid="ignore"):
        m = np.where((bh > bw) | np.isnan(bh), bh, bw)
        if train:
            u = dzi_draws_numpy(box.shape[0], seed) if u is None else np.asarray(u, dtype=f32)
            cx = cx + bw * (f32(shift_ratio) * u[:, 1])
            cy = cy + bh * (f32(shift_ratio) * u[:, 2])
            scale = (m * (f32(1.0) + f32(scale_ratio) * u[:, 0])) * f32(pad_ratio)
        else:
            scale = m * f32(pad_ratio)
        scale = np.where(scale > f32(max(im_hw)), f32(max(im_hw)), scale)
    return np.stack([cx, cy], axis=1).astype(f32), scale.astype(f32)


def dzi_boxes(bbox_xyxy, im_hw, pad_ratio=1.5, scale_ratio=0.25, shift_ratio=0.25, train=False, generator=None, jitter="torch", seed=0):
    """`aug_bbox_DZI` (linemod_pbr.py:99-120) for a batch, on the boxes' device: bbox_xyxy f32[B,4] = (x1,y1,x2,y2) ->
    center f32[B,2] = (cx,cy), scale f32[B], the side of the square source window.  The box is padded by pad_ratio; with `train`
    its side is scaled by 1 + scale_ratio * U(-1,1) and its centre shifted by shift_ratio * U(-1,1) of the box's width / height.
    scale <= max(H, W).  jitter="torch" (the default): torch arithmetic, the three draws per box from `generator`.  jitter="hash": one
    launch of gdm_dzi_boxes_hip, the same arithmetic on the counter-based draws of include/gdm.h from `seed`, an int or a
    one-element int32 device tensor read when the kernel runs (no generator state: the call captures in a graph and a replay draws
    from the word the tensor then holds); `dzi_boxes_numpy` restates it."""
    if jitter not in ("torch", "hash"):
        raise ValueError("jitter must be 'torch' or 'hash', got %r" % (jitter,))
    if not isinstance(bbox_xyxy, torch.Tensor) or bbox_xyxy.dim() != 2 or bbox_xyxy.shape[1] != 4:
        raise ValueError("bbox_xyxy must be a tensor [B,4]")
    box = bbox_xyxy.to(torch.float32)
    if jitter == "hash":
        box = ops._dev(box, torch.float32, "bbox_xyxy")
        B = box.shape[0]
        seed_val, seed_ptr = ops._seed_args(seed)
        center = torch.empty((B, 2), dtype=torch.float32, device=box.device)
        scale = torch.empty((B,), dtype=torch.float32, device=box.device)
        call("gdm_dzi_boxes_hip", box, B, float(max(im_hw)), float(pad_ratio), float(scale_ratio), float(shift_ratio), 1 if train else 0,
             seed_val, seed_ptr, center, scale)
        return center, scale
    u = 2.0 * torch.rand((box.shape[0], 3), device=box.device, generator=generator) - 1.0 if train else None
    return _dzi_torch(box, im_hw, pad_ratio, scale_ratio, shift_ratio, u)


def crop_from_boxes(rgb_u8, depth, normals, K, center, scale, S, mask=None):
    """The loader's six crop_resize_by_warp_affine calls (linemod_pbr.py:468-473) in one launch: rgb_u8 u8[B,H,W,3],
    depth f32[B,H,W], normals f32[B,3,H,W], K f32[B,3,3], center f32[B,2], scale f32[B] (source pixels), mask u8[B,H,W] or None ->
    dict(rgb f32[B,3,S,S] colour-normalised, normals f32[B,3,S,S], dpt_xyz f32[B,S,S,3], depth f32[B,S,S], mask u8[B,S,S] with a
    mask).  Bilinear for rgb and normals, nearest for the rest, zeros outside the frame; with scale == S and
    center = (x0 + S/2, y0 + S/2) it is the integer crop at (x0, y0).  normals=None crops no normals (no "normals" in the dict)."""
    rgb_u8 = ops._dev(rgb_u8, torch.uint8, "rgb_u8")
    depth = ops._dev(depth, torch.float32, "depth")
    if normals is not None:
        normals = ops._dev(normals, torch.float32, "normals")
    K = ops._dev(K, torch.float32, "K")
    center = ops._dev(center, torch.float32, "center")
    scale = ops._dev(scale, torch.float32, "scale")
    if depth.dim() != 3:
        raise ValueError("depth must be [B,H,W], got %s" % (tuple(depth.shape),))
    B, H, W = depth.shape
    for t, shape, name in ((rgb_u8, (B, H, W, 3), "rgb_u8"), (normals, (B, 3, H, W), "normals"), (K, (B, 3, 3), "K"),
                           (center, (B, 2), "center"), (scale, (B,), "scale")):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (name, list(shape), tuple(t.shape)))
    dev = depth.device
    out = dict(rgb=torch.empty((B, 3, S, S), dtype=torch.float32, device=dev),
               dpt_xyz=torch.empty((B, S, S, 3), dtype=torch.float32, device=dev),
               depth=torch.empty((B, S, S), dtype=torch.float32, device=dev))
    if normals is not None:
        out["normals"] = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    if mask is not None:
        mask = ops._dev(mask, torch.uint8, "mask")
        if tuple(mask.shape) != (B, H, W):
            raise ValueError("mask must be [B=%d,H=%d,W=%d], got %s" % (B, H, W, tuple(mask.shape)))
        out["mask"] = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    call("gdm_warp_crop_hip", rgb_u8, depth, normals, K, mask, center, scale, B, H, W, int(S), out["rgb"], out.get("normals"), out["dpt_xyz"],
         out["depth"], out.get("mask"))
    return out


def make_inputs_from_boxes(rgb_u8, depth, K, bbox_xyxy, S, n_points, mask=None, train=False, generator=None, normals=None,
                           depth_fill=None, sampler="torch", seed=0, build_pyramid=True, augment=None, jitter="torch"):
    """The whole item from the raw frame: rgb_u8 u8[B,H,W,3], depth f32[B,H,W] (m), K f32[B,3,3], bbox_xyxy f32[B,4], mask
    u8[B,H,W] or None -> the dict of `make_inputs` (rgb, cld_rgb_nrm, choose, dpt_xyz, origin_labels with a mask, the neighbour
    pyramid) plus n_valid i32[B], the number of depth > 1e-6 pixels of each crop (the loader drops a training item below 200,
    linemod_pbr.py:479), and the center f32[B,2] / scale f32[B] it cropped at.  All on the device without a host synchronisation.

    depth_fill=None, the LineMOD item: depth_normals on the frame (unless `normals` f32[B,3,H,W] is given) -> dzi_boxes ->
    crop_from_boxes -> sample_valid_pixels -> assembly -> pyramid.build_pyramid.

    depth_fill="multiscale" / "fast", the YCB-V item (ycbv_pbr.py:458-509): dzi_boxes -> crop_from_boxes without normals ->
    fill_depth on the cropped depth -> depth_normals of the filled crop with the frame's own K (the reference passes fx, fy unchanged)
    -> sample_valid_pixels among the FILLED pixels (filled > 1e-6, which n_valid then counts) -> assembly -> pyramid.  The dict also
    holds depth_filled f32[B,S,S].  As in the reference (:506), cld is gathered from the crop's UNFILLED dpt_xyz, so a point chosen
    inside a filled hole has xyz = (0,0,0) while its normal comes from the filled surface; `normals` is not taken here.

    sampler="torch" (the default) draws the points with sample_valid_pixels from `generator`.  sampler="hash" replaces
    sample_valid_pixels and the assembly on either leg with ONE launch, ops.sample_assemble: the points follow the written rule of
    include/gdm.h (restated as sample_assemble_numpy) from `seed`, an int or a one-element int32 device tensor; `generator` then only
    feeds the box jitter of train=True.  build_pyramid=False leaves the neighbour pyramid to the caller (infer.pipeline_step builds it
    when the dict lacks it).

    jitter="hash" draws the box jitter of train=True from `seed` as well (dzi_boxes(jitter="hash")).  augment=dict(background=(bg_rgb,
    bg_depth, bg_mask) or None, enable=u8[B] or None) is the YCB-V TRAINING item (ycbv_pbr.py:468-477; the LineMOD item applies none):
    it needs depth_fill and a mask, draws from `seed`, and runs augment_crops on the crop before the fill, so the order is crop ->
    augment -> fill_depth of the augmented depth -> normals, sampling and assembly from the result.  The dict's rgb is then the
    augmented crop and depth_aug f32[B,S,S] the depth the fill read.  dpt_xyz stays the unaugmented crop's, as in the reference, whose
    cld is gathered from dpt_xyz_clip: a point chosen on the pasted background has xyz = (0,0,0), like one inside a filled hole.  With
    train=True, jitter="hash", sampler="hash" and a device seed word the whole item captures in torch.cuda.graph."""
    if sampler not in ("torch", "hash"):
        raise ValueError("sampler must be 'torch' or 'hash', got %r" % (sampler,))
    if augment is not None:
        if depth_fill is None or mask is None:
            raise ValueError("augment= is the YCB-V training item: it needs depth_fill and a mask")
        if set(augment) - {"background", "enable"}:
            raise ValueError("augment takes the keys 'background' and 'enable', got %s" % sorted(augment))
    B, H, W = depth.shape
    center, scale = dzi_boxes(bbox_xyxy, (H, W), train=train, generator=generator, jitter=jitter, seed=seed)
    extra = {}
    if depth_fill is None:
        if normals is None:
            normals = depth_normals(depth, K)
        crop = crop_from_boxes(rgb_u8, depth, normals, K, center, scale, S, mask=mask)
        xyz, nrm = crop["dpt_xyz"], crop["normals"]
        valid_depth = crop["depth"]
        if sampler == "torch":
            choose = sample_valid_pixels(xyz, n_points, generator)                   # [B,1,N]
    else:
        if normals is not None:
            raise ValueError("normals= goes with depth_fill=None: the YCB-V item takes its normals from the filled crop")
        crop = crop_from_boxes(rgb_u8, depth, None, K, center, scale, S, mask=mask)
        if augment is not None:
            crop["rgb"], crop["depth"] = augment_crops(crop["rgb"], crop["depth"], mask=crop["mask"], background=augment.get("background"),
                                                       enable=augment.get("enable"), seed=seed)
            extra["depth_aug"] = crop["depth"]
        filled = fill_depth(crop["depth"], mode=depth_fill)
        xyz, nrm = crop["dpt_xyz"], depth_normals(filled, K)
        valid_depth = filled
        if sampler == "torch":
            choose = sample_valid_pixels(xyz, n_points, generator, valid=filled > 1e-6)
        extra["depth_filled"] = filled
    if sampler == "hash":
        ch, cld_rgb_nrm, labels, n_valid = ops.sample_assemble(valid_depth, xyz, crop["rgb"], nrm, n_points, mask=crop.get("mask"),
                                                               seed=seed)
        inputs = dict(rgb=crop["rgb"], cld_rgb_nrm=cld_rgb_nrm, choose=ch.unsqueeze(1), dpt_xyz=xyz, n_valid=n_valid, center=center,
                      scale=scale, **extra)
        if mask is not None:
            inputs["origin_labels"] = labels
        if build_pyramid:
            inputs.update(pyramid.build_pyramid(pyramid.cloud_from_inputs(cld_rgb_nrm), xyz))
        return inputs
    valid = valid_depth > 1e-6
    ch = choose[:, 0].long()
    cld = torch.gather(xyz.reshape(B, S * S, 3), 1, ch[:, :, None].expand(-1, -1, 3))
    rgb_pt = torch.gather(crop["rgb"].reshape(B, 3, S * S), 2, ch[:, None, :].expand(-1, 3, -1))
    nrm_pt = torch.gather(nrm.reshape(B, 3, S * S), 2, ch[:, None, :].expand(-1, 3, -1))
    inputs = dict(rgb=crop["rgb"], cld_rgb_nrm=torch.cat([cld.transpose(1, 2), rgb_pt, nrm_pt], dim=1).contiguous(), choose=choose,
                  dpt_xyz=xyz, n_valid=valid.reshape(B, S * S).sum(dim=1).to(torch.int32), center=center, scale=scale, **extra)
    if mask is not None:
        lab = torch.gather(crop["mask"].reshape(B, S * S), 1, ch)
        inputs["origin_labels"] = torch.where(lab == 255, torch.ones_like(lab), lab)
    if build_pyramid:
        inputs.update(pyramid.build_pyramid(cld.contiguous(), xyz))
    return inputs
