"""From a BOP mesh to the object model file: `obj_%06d_fps.npy`, the f32[>=M,9] table (xyz in mm, rgb 0..255, unit normal) that
SplineCNN_Mesh, dgcnn.load_mesh and train_lm._model_points read, whose row order is a farthest-point ordering: data[:n] is itself a
farthest-point subset for every n.

    python -m geometric_aware_dense_matching_amd.model_prep --models-dir BOP/models --out-dir kps [--obj-ids 1 5 ...]
           [--n-points 8192] [--candidates S] [--seed 0] [--source surface|vertices]

The work runs on the GPU through three entries of include/gdm.h, each defined by a rule written there:
  ops.surface_sample          area-weighted points on the triangles with interpolated colour and normal (ops.surface_sample_tex for a
                              mesh with texture coordinates and a texture image: the colour is fetched from the image)
  ops.furthestsampling_wide   the farthest-point order over all candidates (ops.furthestsampling below FPS_WIDE_MIN_N candidates)
  ops.point_diameter          the exact farthest pair, whose fp64 length is the `diameter` of models_info.json
surface_sample_numpy, fps_numpy and point_diameter_numpy restate the three rules on the CPU, bit for bit; the tests hold the
kernels to them.  The integer face weights (rint(area / max area * 2^24) in fp64) and their cumulative sum are made here, once per
mesh, and are an INPUT of both the kernel and its restatement.

Not pinned: the script that wrote the reference's own files (tools/lm/lmo_1_compute_fps.py, cited by ref/ycbv.py:106) and the files
themselves are not available, so no parity with them is claimed -- only the file's contract (layout, units, nested farthest-point
prefixes) and bit-equality with the written rules.
"""
import argparse
import glob
import json
import os
import re
import warnings

import numpy as np

from .evaluation import load_ply as _load_ply

# Candidates from which the one-launch-per-pick form is taken.  Measured on an MI355X (profiles/model_prep.md): the wide form costs
# 3.9-4.1 us per pick at every n (it is launch-bound); one workgroup costs 3.6 us per pick at n = 8192 and 4.9 us at n = 16384, the
# first measured n at which the wide form wins.
FPS_WIDE_MIN_N = 16384

_M32 = np.uint64(0xffffffff)


def load_ply(path, attributes=True):
    """evaluation.load_ply with the vertex attributes: (verts f64[V,3], faces i32[F,3], normals f32[V,3] or None, colors u8[V,3] or
    None); attributes=False gives (verts, faces) alone."""
    return _load_ply(path, attributes=attributes)


def load_mesh(path, verbose=False):
    """A PLY file as the mesh dict build_model_points and render.SceneMeshes take: verts, faces, normals, colors (each of the last two
    None when the file has none) and, for a file that carries texture coordinates and names an image (`comment TextureFile`) that
    lies beside it, uv f32[F,3,2] and texture u8[H,W,3], with texture_file the path that was read.  An image that is named but
    missing is said aloud (a warning) and the mesh stays untextured; a missing PIL is an error (texture.load_texture)."""
    from . import texture
    verts, faces, normals, colors, uv, name = _load_ply(path, attributes=True, texcoords=True)
    mesh = dict(verts=verts, faces=faces, normals=normals, colors=colors)
    if uv is not None and name:
        image = os.path.join(os.path.dirname(os.path.abspath(path)), name)
        if os.path.exists(image):
            mesh.update(uv=uv, texture=texture.load_texture(image), texture_file=image)
            if verbose:
                print("%s: texture %s (%d x %d)" % (os.path.basename(path), image, mesh["texture"].shape[1], mesh["texture"].shape[0]))
        else:
            warnings.warn("%s names the texture %s, which does not exist: the mesh is read without it" % (path, image))
    return mesh


def vertex_normals_numpy(verts, faces):
    """Area-weighted vertex normals in fp64: the sum of (B - A) x (C - A) over the faces at a vertex, normalised; f64[V,3].  A vertex
    of no face, or of faces that cancel, keeps a zero normal."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    cross = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    nrm = np.zeros_like(verts)
    for k in range(3):
        np.add.at(nrm, faces[:, k], cross)
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.divide(nrm, length, out=np.zeros_like(nrm), where=length > 0)


def face_cdf(verts, faces):
    """i64[F]: the inclusive cumulative sum of the integer face weights rint(area_f / area_max * 2^24), areas in fp64."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    area = 0.5 * np.linalg.norm(np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]), axis=1)
    if not len(area) or not area.max() > 0:
        raise ValueError("the mesh has no face of positive area")
    return np.cumsum(np.rint(area / area.max() * 2.0 ** 24).astype(np.int64), dtype=np.int64)


# ------------------------------------------------------------------------------------------
# the three rules of include/gdm.h, restated
# ------------------------------------------------------------------------------------------
def _mix32(x):
    """lowbias32 on uint64 arrays that hold 32-bit words."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def surface_sample_numpy(verts, faces, vnrm, vrgb, cdf, S, seed=0, _draws=False):
    """THE SAMPLE RULE of gdm_surface_sample_hip (include/gdm.h): f32[S,9] = xyz, rgb, normal, bit-equal to the kernel.  (_draws: also
    the drawn faces and the fp32 weights w0, u, v as [S,1] columns, for surface_sample_tex_numpy.)"""
    verts, vnrm, vrgb = (np.ascontiguousarray(a, dtype=np.float32) for a in (verts, vnrm, vrgb))
    faces, cdf = np.asarray(faces, dtype=np.int64), np.asarray(cdf, dtype=np.int64)
    S = int(S)
    if not 1 <= S < 1 << 31 or len(verts) < 1 or len(faces) < 1 or cdf.shape != (len(faces),) or cdf[-1] <= 0 or (np.diff(cdf) < 0).any():
        raise ValueError("surface_sample_numpy: needs 1 <= S < 2^31, V >= 1, F >= 1 and a non-decreasing cdf[F] that ends above 0")
    s = np.arange(S, dtype=np.uint64)
    base = _mix32(_mix32(np.uint64((int(seed) & 0xffffffff) ^ 0x9e3779b9)) ^ s)
    h = [_mix32(base ^ np.uint64(((j + 1) * 0x9e3779b9) & 0xffffffff)) for j in range(4)]
    # target = floor((h0 << 32 | h1) * total / 2^64) from 32-bit halves
    total = np.uint64(int(cdf[-1]))
    b_hi, b_lo = total >> np.uint64(32), total & _M32
    p0, p1, p2, p3 = h[1] * b_lo, h[1] * b_hi, h[0] * b_lo, h[0] * b_hi
    mid = (p0 >> np.uint64(32)) + (p1 & _M32) + (p2 & _M32)
    target = (p3 + (p1 >> np.uint64(32)) + (p2 >> np.uint64(32)) + (mid >> np.uint64(32))).astype(np.int64)
    f = np.searchsorted(cdf, target, side="right")                         # the first face with cdf[f] > target
    ui, vi = (h[2] >> np.uint64(8)).astype(np.int64), (h[3] >> np.uint64(8)).astype(np.int64)
    flip = ui + vi > 1 << 24
    ui, vi = np.where(flip, (1 << 24) - ui, ui), np.where(flip, (1 << 24) - vi, vi)
    u = (ui.astype(np.float32) * np.float32(2.0 ** -24))[:, None]
    v = (vi.astype(np.float32) * np.float32(2.0 ** -24))[:, None]
    w0 = (np.float32(1) - u) - v
    a, b, c = faces[f, 0], faces[f, 1], faces[f, 2]
    out = np.empty((S, 9), dtype=np.float32)
    for at, src in ((0, verts), (3, vrgb), (6, vnrm)):
        out[:, at:at + 3] = ((w0 * src[a]) + (u * src[b])) + (v * src[c])
    out[:, 3:6] = np.minimum(np.maximum(np.floor(out[:, 3:6] + np.float32(0.5)), np.float32(0)), np.float32(255))
    n = out[:, 6:9]
    length = np.sqrt(((n[:, 0] * n[:, 0]) + (n[:, 1] * n[:, 1])) + (n[:, 2] * n[:, 2]))[:, None]
    out[:, 6:9] = np.divide(n, length, out=n.copy(), where=length > 0)
    return (out, (f, w0, u, v)) if _draws else out


def surface_sample_tex_numpy(verts, faces, vnrm, vrgb, cdf, fuv, tex, row, S, seed=0, flip_v=True):
    """THE SAMPLE RULE of gdm_surface_sample_tex_hip (include/gdm.h): surface_sample_numpy's draws, xyz and normal; rgb = the texture's
    level 0 at the (u, v) interpolated in fp32 from the face corners' fuv f32[F,3,2].  tex u8[T,4], row = (offset, W0, H0, L)."""
    from . import texture
    out, (f, w0, u, v) = surface_sample_numpy(verts, faces, vnrm, vrgb, cdf, S, seed, _draws=True)
    off, W0, H0, L = (int(x) for x in row)
    if W0 == 0:
        return out
    tex = np.asarray(tex)
    if not texture.valid_row(row, len(tex)):
        raise ValueError("surface_sample_tex_numpy: the row %s does not lie inside %d texels" % ((off, W0, H0, L), len(tex)))
    fuv = np.ascontiguousarray(fuv, dtype=np.float32)
    if fuv.shape != (len(faces), 3, 2):
        raise ValueError("surface_sample_tex_numpy: fuv must be [F=%d,3,2], got %s" % (len(faces), fuv.shape))
    t = ((w0 * fuv[f, 0]) + (u * fuv[f, 1])) + (v * fuv[f, 2])            # fp32 [S,2]
    out[:, 3:6] = texture.fetch_numpy(tex, H0, W0, 0, t[:, 0].astype(np.float64), t[:, 1].astype(np.float64), flip_v, offset=off)
    return out


def fps_numpy(xyz, m):
    """THE RULE of gdm_furthestsampling_hip and gdm_fps_wide_hip for one cloud xyz f32[n,3]: i32[m]."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    n, m = len(xyz), int(m)
    if not 1 <= m <= n:
        raise ValueError("fps_numpy: needs 1 <= m <= n, got m=%d n=%d" % (m, n))
    dist = np.full(n, 1e10, dtype=np.float32)
    idx = np.zeros(m, dtype=np.int32)
    for i in range(1, m):
        d = xyz - xyz[idx[i - 1]]
        d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        dist = np.minimum(dist, d2)
        idx[i] = np.argmax(dist)                                           # the first of equal maxima
    return idx


def point_diameter_numpy(xyz):
    """THE RULE of gdm_point_diameter_hip for xyz f32[V,3]: (pair i32[2] with i < j, d2 np.float32)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    V = len(xyz)
    if V < 2:
        raise ValueError("point_diameter_numpy: needs at least two points")
    cols = np.arange(V)
    best, pair = np.float32(-1), (0, 0)
    for i0 in range(0, V, 256):
        d = xyz[i0:i0 + 256, None, :] - xyz[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        d2[cols[None, :] <= np.arange(i0, i0 + len(d2))[:, None]] = -1     # j > i only
        at = int(np.argmax(d2))                                            # row-major first maximum: lowest i, then lowest j
        if d2.flat[at] > best:
            best, pair = d2.flat[at], (i0 + at // V, at % V)
    return np.array(pair, dtype=np.int32), np.float32(best)


# ------------------------------------------------------------------------------------------
# the pipeline
# ------------------------------------------------------------------------------------------
class _DeviceOps:
    """The three steps on the GPU; numpy in, numpy out."""

    @staticmethod
    def _t(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @classmethod
    def surface_sample(cls, verts, faces, vnrm, vrgb, cdf, S, seed):
        from . import ops
        return ops.surface_sample(cls._t(verts), cls._t(faces), cls._t(vnrm), cls._t(vrgb), cls._t(cdf), S, seed).cpu().numpy()

    @classmethod
    def surface_sample_tex(cls, verts, faces, vnrm, vrgb, cdf, fuv, image, S, seed):
        from . import ops, texture
        tex = texture.build_mips(cls._t(image))
        row = (0, image.shape[1], image.shape[0], texture.full_levels(*image.shape[:2]))
        return ops.surface_sample_tex(cls._t(verts), cls._t(faces), cls._t(vnrm), cls._t(vrgb), cls._t(cdf), cls._t(fuv), tex, row, S, seed,
                                      texture.FLIP_V).cpu().numpy()

    @classmethod
    def fps(cls, xyz, m):
        from . import ops
        op = ops.furthestsampling_wide if len(xyz) >= FPS_WIDE_MIN_N else ops.furthestsampling
        return op(cls._t(xyz)[None], m)[0].cpu().numpy()

    @classmethod
    def point_diameter(cls, xyz):
        from . import ops
        pair, d2 = ops.point_diameter(cls._t(xyz))
        return pair.cpu().numpy(), d2.cpu().numpy()[0]


class _NumpyOps:
    """The same three steps on the restatements (the tests' stand-in, and the reference the GPU pipeline is compared with)."""
    surface_sample = staticmethod(surface_sample_numpy)

    @staticmethod
    def surface_sample_tex(verts, faces, vnrm, vrgb, cdf, fuv, image, S, seed):
        from . import texture
        row = (0, image.shape[1], image.shape[0], texture.full_levels(*image.shape[:2]))
        return surface_sample_tex_numpy(verts, faces, vnrm, vrgb, cdf, fuv, texture.build_mips_numpy(image), row, S, seed, texture.FLIP_V)
    fps = staticmethod(fps_numpy)
    point_diameter = staticmethod(point_diameter_numpy)


_impl = _DeviceOps          # the one hook: what runs the three steps


def _mesh_arrays(mesh):
    """-> verts f64, faces i32, normals f32, colors f32 (levels), uv f32[F,3,2] or None, texture u8[H,W,3] or None.  With a texture
    the colours are not read (zeros when the mesh has none): no grey, no warning."""
    from . import texture as _texture
    if not isinstance(mesh, dict):
        mesh = load_mesh(mesh)
    verts, faces, normals, colors = mesh["verts"], mesh["faces"], mesh.get("normals"), mesh.get("colors")
    uv, image = mesh.get("uv"), mesh.get("texture")
    verts, faces = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int32)
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3 or not len(verts) or not len(faces):
        raise ValueError("a mesh needs verts [V,3] and faces [F,3], got %s and %s" % (verts.shape, faces.shape))
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError("face indices %d..%d outside the %d vertices" % (faces.min(), faces.max(), len(verts)))
    if normals is None:
        normals = vertex_normals_numpy(verts, faces)
    if image is not None:
        if uv is None:
            raise ValueError("a mesh with a texture needs uv")
        uv, image = np.asarray(uv, dtype=np.float32), _texture._image(image)
        if uv.shape == (len(verts), 2):
            uv = uv[faces]
        if uv.shape != (len(faces), 3, 2):
            raise ValueError("uv must be [F=%d,3,2] or [V=%d,2], got %s" % (len(faces), len(verts), uv.shape))
        _texture.level_shapes(image.shape[0], image.shape[1])
        if colors is None:
            colors = np.zeros((len(verts), 3), dtype=np.uint8)
    else:
        uv = None
    if colors is None:
        warnings.warn("the mesh has no vertex colours: every rgb channel of the model file becomes 128")
        colors = np.full((len(verts), 3), 128, dtype=np.uint8)
    return verts, faces, np.asarray(normals, dtype=np.float32), np.asarray(colors).astype(np.float32), uv, image


def build_model_points(mesh, n_points, candidates=None, seed=0, source="surface"):
    """The model table of a mesh: f32[n_points,9] = xyz (the mesh's unit: mm in BOP), rgb 0..255, unit normal, rows in
    farthest-point order from candidate 0 -- so the first k rows are the table of n_points = k FOR THE SAME CANDIDATES.
    mesh: a PLY path, or {"verts", "faces"[, "normals", "colors", "uv", "texture"]}.  source "surface": `candidates` (default
    32 * n_points) points drawn on the triangles by area; "vertices": the mesh's own vertices with their attributes (V >= n_points).
    A mesh with "uv" (f32[F,3,2] per face corner, or [V,2]) and "texture" (u8[H,W,3]) -- a PLY that names a TextureFile beside it --
    takes its rgb from the texture (ops.surface_sample_tex); that needs source "surface": a per-corner uv has no single value at a
    vertex."""
    n_points = int(n_points)
    verts, faces, normals, colors, uv, image = _mesh_arrays(mesh)
    if image is not None and source == "vertices":
        raise ValueError("source='vertices' cannot colour a textured mesh (a per-corner uv has no single vertex value): use 'surface'")
    if n_points < 1:
        raise ValueError("n_points=%d must be at least 1" % n_points)
    if source == "surface":
        S = 32 * n_points if candidates is None else int(candidates)
        if S < n_points:
            raise ValueError("candidates=%d is fewer than n_points=%d" % (S, n_points))
        if image is not None:
            cand = _impl.surface_sample_tex(verts.astype(np.float32), faces, normals, colors, face_cdf(verts, faces), uv, image, S, seed)
        else:
            cand = _impl.surface_sample(verts.astype(np.float32), faces, normals, colors, face_cdf(verts, faces), S, seed)
    elif source == "vertices":
        if len(verts) < n_points:
            raise ValueError("source='vertices' needs at least n_points=%d vertices, the mesh has %d" % (n_points, len(verts)))
        cand = np.concatenate([verts.astype(np.float32), colors, normals], axis=1)
    else:
        raise ValueError("source must be 'surface' or 'vertices', got %r" % (source,))
    cand = np.ascontiguousarray(cand, dtype=np.float32)
    order = _impl.fps(np.ascontiguousarray(cand[:, :3]), n_points)
    return np.ascontiguousarray(cand[order.astype(np.int64)])


def model_diameter(verts):
    """The object's diameter as models_info.json records it: the fp64 length of the farthest pair of vertices, the pair chosen by
    ops.point_diameter on the fp32 coordinates."""
    verts = np.asarray(verts, dtype=np.float64)
    pair, _ = _impl.point_diameter(verts.astype(np.float32))
    return float(np.linalg.norm(verts[int(pair[0])] - verts[int(pair[1])]))


def main(argv=None):
    p = argparse.ArgumentParser(description="obj_%06d_fps.npy model files from the PLY meshes of a BOP models directory")
    p.add_argument("--models-dir", required=True, help="directory with obj_%%06d.ply (and models_info.json)")
    p.add_argument("--out-dir", required=True)
    p.add_argument("--obj-ids", type=int, nargs="*", default=None, help="default: every obj_*.ply of --models-dir")
    p.add_argument("--n-points", type=int, default=8192)
    p.add_argument("--candidates", type=int, default=None, help="surface samples the order is taken over (default 32 * n-points)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--source", choices=["surface", "vertices"], default="surface")
    args = p.parse_args(argv)
    ids = args.obj_ids
    if not ids:
        ids = sorted(int(re.search(r"obj_(\d+)\.ply$", f).group(1)) for f in glob.glob(os.path.join(args.models_dir, "obj_*.ply"))
                     if re.search(r"obj_(\d+)\.ply$", f))
    if not ids:
        raise SystemExit("no obj_*.ply in %s" % args.models_dir)
    info = {}
    info_path = os.path.join(args.models_dir, "models_info.json")
    if os.path.exists(info_path):
        with open(info_path) as f:
            info = {int(k): v for k, v in json.load(f).items()}
    os.makedirs(args.out_dir, exist_ok=True)
    for obj in ids:
        mesh = load_mesh(os.path.join(args.models_dir, "obj_%06d.ply" % obj))
        verts, faces = mesh["verts"], mesh["faces"]
        table = build_model_points(mesh, args.n_points, candidates=args.candidates, seed=args.seed, source=args.source)
        out = os.path.join(args.out_dir, "obj_%06d_fps.npy" % obj)
        np.save(out, table)
        diameter = model_diameter(verts)
        line = "obj %d: %d vertices, %d faces -> %s %s, diameter %.6f" % (obj, len(verts), len(faces), out, table.shape, diameter)
        if "diameter" in info.get(obj, {}):
            rec = float(info[obj]["diameter"])
            line += " (models_info.json: %.6f, relative difference %.3e)" % (rec, abs(diameter - rec) / rec)
        if mesh.get("texture_file"):
            line += ", rgb from the texture %s" % mesh["texture_file"]
        print(line)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
