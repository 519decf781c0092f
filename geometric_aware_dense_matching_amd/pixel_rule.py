"""THE PIXEL RULE of include/gdm.h (gdm_render_depth_hip) on the host, once: the definition csrc/gdm_raster.h is tested
against.  evaluation.render_depth_numpy, pose.raster_depth_face_numpy and render.render_frames_numpy draw with it and differ only in
the z-buffer they keep.  Imports nothing but numpy.

  project          the vertices of one pose -> ok, xs, ys, iz (fp64 transform, discard, snapping to 1/256 px, 1 / Z)
  edge             one int64 edge function over pixel coordinates
  covered          the faces the rule does not discard -> face index, clamped box, `inside` mask, fp32 depth of the box
  depth_keys       fp32 depths -> the keys whose unsigned minimum the kernels keep: the depth bits, or bits << 32 | face
"""
import numpy as np

INF_BITS = 0x7F800000          # the bits of +inf: a pixel whose depth bits reach them counts as not drawn


def project(verts64, rt, K, near):
    """verts64 f64[V,3] under the pose rt f64[3,4] and the intrinsics K f64[3,3] (fx, fy, cx, cy only) -> ok bool[V] (in front of
    `near` and inside the snapping range), xs, ys i64[V] (1/256 px; 0 where not ok), iz f64[V] = 1 / Z."""
    x, y, z = verts64[:, 0], verts64[:, 1], verts64[:, 2]
    R, t = rt[:, :3], rt[:, 3]
    with np.errstate(all="ignore"):
        X = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
        Y = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
        Z = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
        u = K[0, 0] * (X / Z) + K[0, 2]
        v = K[1, 1] * (Y / Z) + K[1, 2]
        ok = (Z > near) & (np.abs(u) <= 65536.0) & (np.abs(v) <= 65536.0)
        xs = np.floor(np.where(ok, u, 0.0) * 256.0 + 0.5).astype(np.int64)
        ys = np.floor(np.where(ok, v, 0.0) * 256.0 + 0.5).astype(np.int64)
        iz = 1.0 / Z
    return ok, xs, ys, iz


def edge(xs, ys, a, c, PX, PY):
    """The edge function of a -> c at the points (PX, PY), all in 1/256 px: positive on the inner side of a normalised winding."""
    return (xs[c] - xs[a]) * (PY - ys[a]) - (ys[c] - ys[a]) * (PX - xs[a])


def covered(faces, ok, xs, ys, iz, H, W, start=0, stop=None):
    """The faces [start, stop) of faces i64[F,3] that the rule draws, in index order -> (f, (px0, py0, px1, py1), inside, d): the
    pixel box clamped to the image, inclusive; inside bool[py1-py0+1, px1-px0+1], true somewhere; d f32 of that shape, the
    perspective-correct depth (meaningful where inside).  Discarded: an index outside [0, V), a vertex that is not ok, a snapped area
    of 0, an empty box, no covered pixel."""
    V = len(ok)
    for f in range(start, len(faces) if stop is None else stop):
        i0, i1, i2 = faces[f]
        if not (0 <= i0 < V and 0 <= i1 < V and 0 <= i2 < V) or not (ok[i0] and ok[i1] and ok[i2]):
            continue
        A2 = (xs[i1] - xs[i0]) * (ys[i2] - ys[i0]) - (xs[i2] - xs[i0]) * (ys[i1] - ys[i0])
        if A2 == 0:
            continue
        if A2 < 0:                                                         # normalise the winding: both are drawn
            i1, i2 = i2, i1
        px0, px1 = max((min(xs[i0], xs[i1], xs[i2]) + 255) >> 8, 0), min(max(xs[i0], xs[i1], xs[i2]) >> 8, W - 1)
        py0, py1 = max((min(ys[i0], ys[i1], ys[i2]) + 255) >> 8, 0), min(max(ys[i0], ys[i1], ys[i2]) >> 8, H - 1)
        if px0 > px1 or py0 > py1:
            continue
        PX, PY = np.meshgrid(np.arange(px0, px1 + 1, dtype=np.int64) * 256, np.arange(py0, py1 + 1, dtype=np.int64) * 256)
        inside, w = np.ones(PX.shape, dtype=bool), []
        for a, c in ((i1, i2), (i2, i0), (i0, i1)):                        # the edge opposite vertex 0, 1, 2
            dx, dy = xs[c] - xs[a], ys[c] - ys[a]
            e = edge(xs, ys, a, c, PX, PY)
            inside &= (e > 0) | ((e == 0) & bool(dy < 0 or (dy == 0 and dx > 0)))          # the top-left rule
            w.append(e)
        if not inside.any():
            continue
        A = ((w[0] + w[1]) + w[2]).astype(np.float64)
        with np.errstate(all="ignore"):
            izp = ((w[0].astype(np.float64) * iz[i0] + w[1].astype(np.float64) * iz[i1]) + w[2].astype(np.float64) * iz[i2]) / A
            d = (1.0 / izp).astype(np.float32)
        yield f, (int(px0), int(py0), int(px1), int(py1)), inside, d


def depth_keys(d, face=None):
    """d f32[...] -> the z-buffer keys of the kernels: u32 depth bits (positive floats order like their bits; NaN and negative values
    lie above +inf), or with `face` u64 bits << 32 | face, so that equal depths go to the lower face.  The kernels keep the unsigned
    minimum; np.minimum on these keys is that."""
    bits = np.ascontiguousarray(d).view(np.uint32)
    return bits if face is None else (bits.astype(np.uint64) << np.uint64(32)) | np.uint64(face)
