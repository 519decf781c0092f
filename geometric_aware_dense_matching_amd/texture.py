"""Texture maps: THE TEXTURE RULE of include/gdm.h on the host, once, and the device pyramid builder.

  load_texture       an image file -> u8[H,W,3] (PIL, loaded only when a texture is named; a clear error without it)
  build_mips         u8[H,W,3] on the device -> the pyramid, u8[T,4] texels (gdm_texture_mips_hip)
  build_mips_numpy   the same on the host, bit for bit
  level_shapes       the (H_l, W_l) of the levels; pyramid_texels their sum
  fetch_numpy        Fetch(level, u, v): bilinear with 8-bit fractions, integer blend, clamp to edge -> u8[...,3]
  mip_level_numpy    the level of a pixel from its (U, V) and its two neighbours', without a transcendental
  pack_table         pyramids of several objects -> one texel buffer and the table i64[O,4] = (offset, W0, H0, L)

render.render_frames_numpy and model_prep.surface_sample_tex_numpy fetch with it; the kernels' copy is csrc/gdm_texture.h.  flip_v=True
(the default of a definition) makes v = 0 the image's bottom row.
"""
import numpy as np

MAX_SIDE = 16384
FLIP_V = True


def load_texture(path):
    """The image at `path` as u8[H,W,3] (alpha dropped, palettes and grey expanded).  Needs PIL; says so when it is missing."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("the mesh names the texture %s and reading it needs PIL (pillow), which is not installed: %s" % (path, e))
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def full_levels(H, W):
    """1 + floor(log2(max(W, H))): down to the level whose larger side is 1."""
    return int(max(int(H), int(W))).bit_length()


def level_shapes(H, W, L=None):
    """[(H_l, W_l)] of levels 0 .. L-1 of an H x W image (L defaults to all of them)."""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("a texture is [1, %d] texels each way, got %d x %d" % (MAX_SIDE, W, H))
    L = full_levels(H, W) if L is None else int(L)
    if not 1 <= L <= full_levels(H, W):
        raise ValueError("L=%d not in [1, %d] for a %d x %d texture" % (L, full_levels(H, W), W, H))
    return [(max(1, H >> l), max(1, W >> l)) for l in range(L)]


def pyramid_texels(H, W, L=None):
    return sum(h * w for h, w in level_shapes(H, W, L))


def _image(image):
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise ValueError("a texture is u8[H,W,3], got %s %s" % (image.dtype, image.shape))
    return image


def build_mips_numpy(image, L=None):
    """THE TEXTURE RULE's storage and mips: u8[T,4] = the levels one after the other, texels (r, g, b, 0)."""
    image = _image(image)
    shapes = level_shapes(image.shape[0], image.shape[1], L)
    levels = [image.astype(np.int64)]
    for h, w in shapes[1:]:
        src = levels[-1]
        ya, yb = np.minimum(2 * np.arange(h), src.shape[0] - 1), np.minimum(2 * np.arange(h) + 1, src.shape[0] - 1)
        xa, xb = np.minimum(2 * np.arange(w), src.shape[1] - 1), np.minimum(2 * np.arange(w) + 1, src.shape[1] - 1)
        levels.append((src[ya][:, xa] + src[ya][:, xb] + src[yb][:, xa] + src[yb][:, xb] + 2) >> 2)
    out = np.zeros((sum(h * w for h, w in shapes), 4), dtype=np.uint8)
    at = 0
    for lv in levels:
        out[at:at + lv.shape[0] * lv.shape[1], :3] = lv.reshape(-1, 3)
        at += lv.shape[0] * lv.shape[1]
    return out


def build_mips(image, L=None):
    """The pyramid of a device image u8[H,W,3] on the device: u8[T,4] (gdm_texture_mips_hip)."""
    from . import ops
    return ops.texture_mips(image, L)


def level_view(pyr, H, W, level, offset=0):
    """Level `level` of a pyramid (u8[T,4], starting `offset` texels into it) of an H x W image as u8[H_l,W_l,4]."""
    shapes = level_shapes(H, W, level + 1)
    at = offset + sum(h * w for h, w in shapes[:-1])
    h, w = shapes[-1]
    return pyr[at:at + h * w].reshape(h, w, 4)


def _axis(c, n):
    x = c * float(n) - 0.5
    x0 = np.floor(x)
    fr = np.floor((x - x0) * 256.0).astype(np.int64)
    b = np.minimum(np.maximum(x0, -1.0), float(n)).astype(np.int64)
    return np.clip(b, 0, n - 1), np.clip(b + 1, 0, n - 1), fr


def fetch_numpy(pyr, H, W, level, u, v, flip_v=FLIP_V, offset=0):
    """Fetch(level, u, v) of THE TEXTURE RULE for arrays u, v (fp64) on the pyramid of an H x W image: u8[...,3]."""
    u, v = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
    lv = level_view(pyr, H, W, int(level), offset).astype(np.int64)
    hl, wl = lv.shape[:2]
    finite = np.isfinite(u) & np.isfinite(v)
    uu, vv = np.where(finite, u, 0.0), np.where(finite, v, 0.0)
    with np.errstate(all="ignore"):
        x0, x1, fx = _axis(uu, wl)
        y0, y1, fy = _axis(1.0 - vv if flip_v else vv, hl)
    fx, fy = fx[..., None], fy[..., None]
    top = lv[y0, x0, :3] * (256 - fx) + lv[y0, x1, :3] * fx
    bot = lv[y1, x0, :3] * (256 - fx) + lv[y1, x1, :3] * fx
    out = (top * (256 - fy) + bot * fy + 32768) >> 16
    return np.where(finite[..., None], out, lv[0, 0, :3]).astype(np.uint8)


def mip_level_numpy(U, V, Ux, Vx, Uy, Vy, L, fine=True):
    """The level of THE TEXTURE RULE: (U, V) = (u W0, v H0) at the pixel, (Ux, Vx) at (px + 1, py), (Uy, Vy) at (px, py + 1), fp64
    arrays; `fine` false where a neighbour's Q is not > 0 (the coarsest level).  -> i64[...], the smallest l with rho2 <= 4^l, capped
    at L - 1."""
    U, V, Ux, Vx, Uy, Vy, fine = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (U, V, Ux, Vx, Uy, Vy)],
                                                     np.asarray(fine, dtype=bool))
    with np.errstate(all="ignore"):
        dUx, dVx, dUy, dVy = Ux - U, Vx - V, Uy - U, Vy - V
        a, b = dUx * dUx + dVx * dVx, dUy * dUy + dVy * dVy
        rho2 = np.where(a >= b, a, np.where(b > a, b, a + b))              # the larger; NaN if either is
        level = np.zeros(rho2.shape, dtype=np.int64)
        t = 1.0
        for l in range(int(L) - 1):                                        # still at l and rho2 above 4^l (or NaN): one level up
            level += ~(rho2 <= t) & (level == l)
            t *= 4.0
    return np.where(fine, level, int(L) - 1)


def pack_table(textures):
    """textures: one u8[H,W,3] or None per object -> (tex u8[T,4] with T >= 1, tab i64[O,4] = (offset, W0, H0, L)); an object
    without a texture gets the row (0, 0, 0, 0)."""
    parts, tab, at = [], [], 0
    for t in textures:
        if t is None:
            tab.append((0, 0, 0, 0))
            continue
        t = _image(t)
        pyr = build_mips_numpy(t)
        tab.append((at, t.shape[1], t.shape[0], full_levels(*t.shape[:2])))
        parts.append(pyr)
        at += len(pyr)
    tex = np.concatenate(parts) if parts else np.zeros((1, 4), dtype=np.uint8)
    return np.ascontiguousarray(tex), np.asarray(tab, dtype=np.int64).reshape(-1, 4)


def valid_row(row, tex_texels):
    """What the kernels accept of a table row (offset, W0, H0, L) against a buffer of tex_texels texels."""
    off, W0, H0, L = (int(x) for x in row)
    if not (1 <= W0 <= MAX_SIDE and 1 <= H0 <= MAX_SIDE) or not 1 <= L <= full_levels(H0, W0):
        return False
    return 0 <= off <= tex_texels and pyramid_texels(H0, W0, L) <= tex_texels - off
