"""A structured-light depth sensor on a metric depth frame (gdm_depth_sensor_hip): range limits, the projector's
shadow, drop-outs at grazing incidence, a pixel of lateral jitter, disparity noise and quantisation -- THE SENSOR RULE of
include/gdm.h, a function of the depth frame alone.

  DepthSensor                    the parameter record; `stages` takes names
  simulate_depth_sensor          depth f32[n,H,W] on the device -> dict(depth, cause), one launch
  simulate_depth_sensor_numpy    the rule on the host, operation for operation in np.float32; the kernel equals it bit for bit

baseline 0.075 m and subpixel 8 (1/8 pixel of disparity) are the published Kinect v1 figures.  sigma_d, cos_min, cos_soft, p_shift,
z_min and z_max are the defaults of a definition, not tuned values: no parity with a real device, with BlenSor or with simkinect is
claimed.  cause: 0 measured, 1 empty in the input, 2 out of range, 3 projector shadow, 4 grazing, 5 jittered onto a pixel outside
the frame.
"""
import numpy as np

STAGES = {"range": 1, "shadow": 2, "grazing": 4, "jitter": 8, "noise": 16}          # GDM_SENSOR_RANGE .. GDM_SENSOR_NOISE
ALL_STAGES = 31
CAUSES = ("measured", "empty", "range", "shadow", "grazing", "outside")
MAX_DISP = 255          # GDM_SENSOR_MAX_DISP
MAX_K = 64              # GDM_SENSOR_MAX_K
_STREAM = 0x27D4EB2F
_UNIT = np.float32(0.0067658751)          # 1 / sqrt(21845): the Irwin-Hall integer to unit variance


def tile_shape():
    """(GDM_SENSOR_TILE_W, GDM_SENSOR_TILE_H) of include/gdm.h: the pixels one workgroup of the kernel owns."""
    from . import ops
    assert ops.SENSOR["GDM_SENSOR_MAX_DISP"] == MAX_DISP and ops.SENSOR["GDM_SENSOR_MAX_K"] == MAX_K
    assert all(ops.SENSOR["GDM_SENSOR_" + k.upper()] == v for k, v in STAGES.items())
    return ops.SENSOR["GDM_SENSOR_TILE_W"], ops.SENSOR["GDM_SENSOR_TILE_H"]


def stage_mask(stages):
    """"all", an int in [0, 31], one name or an iterable of names out of STAGES -> the bit mask."""
    if isinstance(stages, str):
        stages = ALL_STAGES if stages == "all" else (stages,)
    if isinstance(stages, (int, np.integer)):
        if not 0 <= int(stages) <= ALL_STAGES:
            raise ValueError("stages=%d not in [0, %d]" % (stages, ALL_STAGES))
        return int(stages)
    mask = 0
    for s in stages:
        if s not in STAGES:
            raise ValueError("unknown sensor stage %r (known: %s)" % (s, ", ".join(STAGES)))
        mask |= STAGES[s]
    return mask


class DepthSensor:
    """The parameters of THE SENSOR RULE.  baseline (metres, signed: the projector sits at camera x = +baseline, the shadow of an
    occluder falls on its left for a positive one), z_min / z_max (metres), sigma_d (disparity noise, pixels), subpixel (disparity
    steps per pixel), cos_min / cos_soft (a surface whose incidence cosine is below cos_min always drops, above cos_soft never, in
    between with a probability linear in the squared cosine), p_shift (the probability that a pixel reads its neighbour, per axis),
    stages ("all", names out of sensor.STAGES, or the bit mask)."""
    __slots__ = ("baseline", "z_min", "z_max", "sigma_d", "subpixel", "cos_min", "cos_soft", "p_shift", "stages")

    def __init__(self, baseline=0.075, z_min=0.4, z_max=4.0, sigma_d=0.125, subpixel=8.0, cos_min=0.1, cos_soft=0.35, p_shift=0.2,
                 stages="all"):
        self.baseline, self.z_min, self.z_max, self.sigma_d = float(baseline), float(z_min), float(z_max), float(sigma_d)
        self.subpixel, self.cos_min, self.cos_soft, self.p_shift = float(subpixel), float(cos_min), float(cos_soft), float(p_shift)
        self.stages = stage_mask(stages)

    def scalars(self):
        return (self.baseline, self.z_min, self.z_max, self.sigma_d, self.subpixel, self.cos_min, self.cos_soft, self.p_shift)

    def replace(self, **kw):
        d = {k: getattr(self, k) for k in self.__slots__}
        d.update(kw)
        return DepthSensor(**d)

    def __repr__(self):
        return "DepthSensor(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def _host_K(K, n):
    """K (numpy, a host tensor, or a device tensor -- the one case that reads the device) -> a host float32 tensor [3,3] or [n,3,3]."""
    import torch
    if torch.is_tensor(K):
        K = K.detach().to(device="cpu", dtype=torch.float32)
    else:
        K = torch.from_numpy(np.ascontiguousarray(np.asarray(K, dtype=np.float32)))
    if tuple(K.shape) not in ((3, 3), (n, 3, 3)):
        raise ValueError("K must be [3,3] or [n=%d,3,3], got %s" % (n, tuple(K.shape)))
    if K.dim() == 3 and n > 1 and bool((K == K[0]).all()):          # one camera: its K travels once, whatever n
        K = K[0]
    return K.contiguous()


def simulate_depth_sensor(depth, K, sensor=None, seed=0):
    """THE SENSOR RULE on the device, one launch: depth f32[n,H,W] (metres; 0, negative or NaN = no depth), K [3,3] or [n,3,3] as
    numpy or a host tensor (a device tensor is copied to the host first: the shadow window is checked before the launch), sensor a
    DepthSensor (default DepthSensor()), seed an int or a one-element int32 device tensor read when the kernel runs ->
    dict(depth f32[n,H,W], cause u8[n,H,W]) on the device.  No host synchronisation with K on the host; captures in a hipGraph.
    With differing K per frame n <= MAX_K."""
    from . import ops
    sensor = DepthSensor() if sensor is None else sensor
    if depth.dim() != 3:
        raise ValueError("depth must be [n,H,W], got %s" % (tuple(depth.shape),))
    out_depth, cause = ops.depth_sensor(depth, _host_K(K, depth.shape[0]), *sensor.scalars(), sensor.stages, seed=seed)
    return dict(depth=out_depth, cause=cause)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _mix32(x):
    from .frontend import _mix32 as mix
    return mix(np.atleast_1d(np.asarray(x, dtype=np.uint32)))


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` where that lies outside."""
    H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        out[yd, xd] = a[ys, xs]
    return out


def frame_constants(K, sensor):
    """(fx, fy, cx, cy, fb, Wd) of one frame as the rule computes them; refuses what the library refuses."""
    f32 = np.float32
    K = np.asarray(K, dtype=f32)
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0):
        raise ValueError("K: fx=%r, fy=%r must be positive and finite" % (fx, fy))
    fb = f32(float(fx) * float(abs(f32(sensor.baseline))))                 # fp64, rounded once
    w = np.ceil(fb / f32(sensor.z_min))
    if not 1 <= w <= MAX_DISP:
        raise ValueError("the shadow window ceil(fx |baseline| / z_min) = %r not in [1, %d]" % (w, MAX_DISP))
    return fx, fy, cx, cy, fb, int(w)


def _check(sensor):
    s = sensor
    f = np.float32
    ok = (np.isfinite(f(s.baseline)) and f(s.baseline) != 0 and np.isfinite(f(s.z_min)) and f(s.z_min) > 0 and f(s.z_max) > f(s.z_min)
          and np.isfinite(f(s.sigma_d)) and f(s.sigma_d) >= 0 and np.isfinite(f(s.subpixel)) and f(s.subpixel) >= 1
          and 0 <= f(s.cos_min) <= f(s.cos_soft) <= 1 and 0 <= f(s.p_shift) <= 1)
    if not ok:
        raise ValueError("%r: outside the limits of THE SENSOR RULE (include/gdm.h)" % (sensor,))


def simulate_depth_sensor_numpy(depth, K, sensor=None, seed=0, return_stages=False):
    """THE SENSOR RULE of include/gdm.h on the host, operation for operation in np.float32: depth [n,H,W], K [3,3] or [n,3,3] ->
    dict(depth f32[n,H,W], cause u8[n,H,W]).  return_stages=True adds what the rule computes on the way: jx, jy i8[n,H,W] (the drawn
    shift, 0 with the stage off), disp and disp_noisy f32[n,H,W] (D and D' of stage 5 where it ran, NaN elsewhere)."""
    f32, u32 = np.float32, np.uint32
    sensor = DepthSensor() if sensor is None else sensor
    _check(sensor)
    depth = np.asarray(depth, dtype=f32)
    if depth.ndim != 3:
        raise ValueError("depth must be [n,H,W], got %s" % (depth.shape,))
    n, H, W = depth.shape
    K = np.asarray(K.detach().cpu().numpy() if hasattr(K, "detach") else K, dtype=f32)
    K = np.broadcast_to(K, (n, 3, 3))
    st = sensor.stages
    z_min, z_max, sigma_d, subpixel = f32(sensor.z_min), f32(sensor.z_max), f32(sensor.sigma_d), f32(sensor.subpixel)
    cmin2, csoft2 = f32(sensor.cos_min) * f32(sensor.cos_min), f32(sensor.cos_soft) * f32(sensor.cos_soft)
    t_shift = u32(int(f32(sensor.p_shift) * f32(32768.0)))
    neg = f32(sensor.baseline) < 0
    out = np.zeros((n, H, W), dtype=f32)
    cause_out = np.zeros((n, H, W), dtype=np.uint8)
    extra = dict(jx=np.zeros((n, H, W), np.int8), jy=np.zeros((n, H, W), np.int8), disp=np.full((n, H, W), np.nan, f32),
                 disp_noisy=np.full((n, H, W), np.nan, f32))
    xi, yi = np.meshgrid(np.arange(W), np.arange(H))
    xs, ys = xi.astype(f32), yi.astype(f32)
    p = (yi * W + xi).astype(u32)
    for b in range(n):
        fx, fy, cx, cy, fb, wd = frame_constants(K[b], sensor)
        hb = _mix32(_mix32(u32(seed & 0xFFFFFFFF) ^ u32(_STREAM)) ^ u32(b))
        hs1, hs2, hs3 = (_mix32(hb ^ u32(s)) for s in (1, 2, 3))
        z = depth[b]
        with np.errstate(all="ignore"):
            valid = z > 0
            cause = np.where(valid, 0, 1).astype(np.uint8)
            surv = valid.copy()
            if st & STAGES["range"]:
                oor = valid & ~((z >= z_min) & (z <= z_max))
                cause[oor] = 2
                surv &= ~oor
            zs = np.where(surv, z, f32(1.0))                               # a placeholder where nothing survives; never used there
            D = fb / zs
            alive = surv.copy()
            if st & STAGES["shadow"]:
                g = xs + D if neg else xs - D
                shadowed = np.zeros((H, W), dtype=bool)
                for d in range(1, min(wd, W - 1) + 1):
                    both = surv[:, d:] & surv[:, :-d]
                    if neg:                                                # x' = x - d shadows x
                        shadowed[:, d:] |= both & (g[:, :-d] >= g[:, d:])
                    else:                                                  # x' = x + d shadows x
                        shadowed[:, :-d] |= both & (g[:, d:] <= g[:, :-d])
                cause[shadowed] = 3
                alive &= ~shadowed
            if st & STAGES["grazing"]:
                u, v = (xs - cx) / fx, (ys - cy) / fy
                P = (zs * u, zs * v, zs)
                sl, sr, su, sd = (_shift(surv, dy, dx, False) for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)))
                Pl, Pr, Pu, Pd = ([_shift(c, dy, dx, f32(0)) for c in P] for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)))
                tx = [np.where(sl & sr, r - l, np.where(sr, r - c, c - l)) for l, r, c in zip(Pl, Pr, P)]
                ty = [np.where(su & sd, dn - up, np.where(sd, dn - c, c - up)) for up, dn, c in zip(Pu, Pd, P)]
                have = (sl | sr) & (su | sd)
                nrm = (tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0])

                def dot(a, c):
                    return (a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]
                npd = dot(nrm, P)
                c2 = (npd * npd) / (dot(nrm, nrm) * dot(P, P))
                hard = ~(c2 >= cmin2)
                soft = ~hard & (c2 < csoft2)
                r = np.where(soft, (csoft2 - c2) / (csoft2 - cmin2), f32(0))
                T = (r * f32(16777216.0)).astype(u32)
                word = _mix32(hs1 ^ p)
                drop = alive & (~have | hard | (soft & ((word >> u32(8)) < T)))
                cause[drop] = 4
                alive &= ~drop
            # stage 4
            jx = np.zeros((H, W), dtype=np.int64)
            jy = np.zeros((H, W), dtype=np.int64)
            if st & STAGES["jitter"]:
                w = _mix32(hs2 ^ p)
                h0, h1 = w & u32(0xFFFF), w >> u32(16)
                hi = u32(65536) - t_shift
                jx = np.where(h0 < t_shift, -1, np.where(h0 >= hi, 1, 0))
                jy = np.where(h1 < t_shift, -1, np.where(h1 >= hi, 1, 0))
            qx, qy = xi + jx, yi + jy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            cq = np.where(inside, cause[qyc, qxc], 5).astype(np.uint8)
            zq = np.where(alive, z, f32(0))[qyc, qxc]
            meas = cq == 0
            o = np.where(meas, zq, f32(0))
            if st & STAGES["noise"]:
                zq1 = np.where(meas, zq, f32(1.0))
                Dq0 = fb / zq1
                w = _mix32(hs3 ^ p)
                zeta = ((w & u32(255)) + ((w >> u32(8)) & u32(255)) + ((w >> u32(16)) & u32(255)) + (w >> u32(24))).astype(np.int64) - 510
                e = zeta.astype(f32) * _UNIT
                Dn = Dq0 + sigma_d * e
                Dq = np.rint(Dn * subpixel) / subpixel
                bad = meas & ~(Dq > 0)
                cq[bad] = 2
                o = np.where(meas & ~bad, fb / np.where(Dq > 0, Dq, f32(1.0)), f32(0))
                extra["disp"][b] = np.where(meas, Dq0, f32(np.nan))
                extra["disp_noisy"][b] = np.where(meas, Dn, f32(np.nan))
        out[b], cause_out[b] = o.astype(f32), cq
        extra["jx"][b], extra["jy"][b] = jx, jy
    res = dict(depth=out, cause=cause_out)
    if return_stages:
        res.update(extra)
    return res
