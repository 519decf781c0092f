"""RGB-D training frames from triangle meshes on the GPU (gdm_render_frames_hip), and training batches made of them.

  SceneMeshes            O meshes packed into one vertex / face table (on the device, and on the host for the restatement); a mesh
                         may carry uv per face corner and a texture image (texture.py; gdm_render_frames_tex_hip)
  render_frames          n frames of S posed objects -> rgb, depth, inst, face, px_all, px_vis, bbox_vis, visib_fract (two kernels)
  render_frames_numpy    the written rule of include/gdm.h on the host, bit for bit, plus `ambiguous` (where the rule's minimum is
                         decided by less than 2 fp32 ulp of depth, so a one-ulp difference in a division could change the winner)
  demo_mesh              a bumpy, coloured subdivided icosahedron, about 0.1 across: an object to train on without any file
                         (textured=True: the same solid with a seamed spherical uv and a hash-drawn image instead of vertex colours)
  backdrop_mesh          a coloured vertex-grid plane behind the objects, so that a frame has valid depth everywhere
  sample_scene_poses     counter-based pose draws on the host: the target in slot 0, distractors (some in front of it) in the others
  RenderedFrames         an iterable of training batches: poses -> render -> frontend.make_inputs_from_boxes -> + RT; the labels,
                         match_idx and visible_flag then come from train_lm.device_targets

Lengths stay in the caller's unit (depth comes out in it); the training chain wants metres.  Parity with BOP's renderers or with
BlenderProc's PBR frames is not claimed: the frame is defined by the written rule.
"""
import numpy as np
import torch

from . import pixel_rule

NEAR = 0.01
AMBIENT = 0.4
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_NO_DEPTH = 0xFFFFFFFF


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
class SceneMeshes:
    """A list of meshes, each (verts [V,3], faces [F,3], colours u8[V,3] or None, normals [V,3] or None) -- the order of
    `model_prep.load_ply(path)` is (verts, faces, normals, colours): use `SceneMeshes.from_ply` for files --, concatenated:
    verts f32 (or f64 with verts_dtype) [Vt,3], vcol u8[Vt,3], vnrm f32[Vt,3], faces i32[Ft,3] indexing the concatenated vertices,
    obj_face0 = the O+1 face offsets.  Missing normals are model_prep.vertex_normals_numpy's, missing colours grey (128).  `scale`
    multiplies the vertices (0.001: a BOP mesh in mm -> metres).  device=None keeps the host arrays only (the restatement's input).
    A mesh tuple may carry a 5th and a 6th item, uv f32[F,3,2] (one (u, v) per face corner; or per vertex, [V,2], gathered through
    the faces) and texture u8[H,W,3]: the object is then coloured from the texture by THE TEXTURE RULE of include/gdm.h (texture.py)
    and its vertex colours are not read.  The scene packs fuv f32[Ft,3,2] (zeros for the other objects), every pyramid into one
    texel buffer tex u8[T,4] and tex_tab i64[O,4] = (offset, W0, H0, L), all zero for an object without a texture; has_texture says
    whether any object has one, flip_v (texture.FLIP_V) is the scene's reading of v."""

    def __init__(self, meshes, device="cuda", verts_dtype=np.float32, scale=1.0, flip_v=None):
        from . import model_prep, texture
        if not meshes:
            raise ValueError("SceneMeshes needs at least one mesh")
        verts, faces, cols, nrms, face0, v0 = [], [], [], [], [0], 0
        fuvs, textures = [], []
        for k, m in enumerate(meshes):
            v, f = np.asarray(m[0], dtype=np.float64) * float(scale), np.asarray(m[1]).astype(np.int64)
            c = m[2] if len(m) > 2 else None
            nr = m[3] if len(m) > 3 else None
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or len(v) < 1 or len(f) < 1:
                raise ValueError("mesh %d: verts must be [V,3] and faces [F,3], got %s and %s" % (k, v.shape, f.shape))
            if f.min() < 0 or f.max() >= len(v):
                raise ValueError("mesh %d: a face index lies outside [0, %d)" % (k, len(v)))
            nr = model_prep.vertex_normals_numpy(v, f) if nr is None else np.asarray(nr)
            c = np.full((len(v), 3), 128, dtype=np.uint8) if c is None else np.asarray(c)
            if c.shape != v.shape or nr.shape != v.shape:
                raise ValueError("mesh %d: colours and normals must be [V=%d,3]" % (k, len(v)))
            uv = m[4] if len(m) > 4 else None
            tx = m[5] if len(m) > 5 else None
            if tx is not None:
                if uv is None:
                    raise ValueError("mesh %d: a texture needs uv" % k)
                uv = np.asarray(uv, dtype=np.float32)
                if uv.shape == (len(v), 2):
                    uv = uv[f]
                if uv.shape != (len(f), 3, 2):
                    raise ValueError("mesh %d: uv must be [F=%d,3,2] or [V=%d,2], got %s" % (k, len(f), len(v), uv.shape))
                tx = texture._image(tx)
                texture.level_shapes(tx.shape[0], tx.shape[1])          # refuses a side outside [1, 16384]
            fuvs.append(np.zeros((len(f), 3, 2), dtype=np.float32) if tx is None else uv)
            textures.append(tx)
            verts.append(v)
            faces.append(f + v0)
            cols.append(np.clip(np.floor(c.astype(np.float64) + 0.5), 0, 255).astype(np.uint8))
            nrms.append(nr.astype(np.float32))
            v0 += len(v)
            face0.append(face0[-1] + len(f))
        self.verts_np = np.ascontiguousarray(np.concatenate(verts).astype(verts_dtype))
        self.vcol_np = np.ascontiguousarray(np.concatenate(cols))
        self.vnrm_np = np.ascontiguousarray(np.concatenate(nrms))
        self.faces_np = np.ascontiguousarray(np.concatenate(faces).astype(np.int32))
        self.obj_face0 = face0
        self.n_objects = len(meshes)
        self.has_texture = any(t is not None for t in textures)
        self.flip_v = texture.FLIP_V if flip_v is None else bool(flip_v)
        self.fuv_np = np.ascontiguousarray(np.concatenate(fuvs))
        self.tex_np, self.tex_tab_np = texture.pack_table(textures)
        self.device = None if device is None else torch.device(device)
        if self.device is not None:
            self.verts, self.vcol, self.vnrm, self.faces = (torch.from_numpy(a).to(self.device) for a in
                                                            (self.verts_np, self.vcol_np, self.vnrm_np, self.faces_np))
            if self.has_texture:                                           # the pyramids are built on the device, image by image
                self.fuv, self.tex_tab = torch.from_numpy(self.fuv_np).to(self.device), torch.from_numpy(self.tex_tab_np).to(self.device)
                self.tex = torch.cat([texture.build_mips(torch.from_numpy(t).to(self.device)) for t in textures if t is not None])

    @classmethod
    def from_ply(cls, paths, **kw):
        """The meshes of PLY files; a file that names a texture (`comment TextureFile`) and carries uv is drawn with the image of that
        name beside it (model_prep.load_mesh)."""
        from . import model_prep
        return cls([_as_mesh(model_prep.load_mesh(p)) for p in paths], **kw)


def _as_mesh(m):
    """A mesh dict (demo_mesh, backdrop_mesh, model_prep.load_mesh) as the tuple SceneMeshes takes."""
    return (m["verts"], m["faces"], m.get("colors"), m.get("normals"), m.get("uv"), m.get("texture"))


def _np(a, dtype):
    return np.ascontiguousarray((a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(dtype))


def _light(light, n):
    light = np.array([0.0, 0.0, -1.0]) if light is None else _np(light, np.float64)          # towards the camera: a head light
    return np.broadcast_to(light, (n, 3)).copy()


def _outputs(rgb, depth, inst, face, stats, xp):
    px_all, px_vis = stats[..., 0], stats[..., 1]
    if xp is torch:
        fract = torch.where(px_all > 0, px_vis.float() / px_all.clamp(min=1).float(), torch.zeros_like(px_vis, dtype=torch.float32))
    else:
        fract = np.where(px_all > 0, px_vis.astype(np.float32) / np.maximum(px_all, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return dict(rgb=rgb, depth=depth, inst=inst, face=face, px_all=px_all, px_vis=px_vis, bbox_vis=stats[..., 2:6], visib_fract=fract)


def render_frames(scene, slot_obj, RT, K, H, W, light=None, ambient=AMBIENT, near=NEAR):
    """n frames of S posed objects of `scene` on the device: slot_obj int[n,S] (object index, -1 = empty slot), RT [n,S,3,4] (object
    -> camera), K [3,3] or [n,3,3], light [3] or [n,3] (unit, camera frame, from the surface towards the light; default the head
    light (0, 0, -1)) -> dict of device tensors: rgb u8[n,H,W,3], depth f32[n,H,W] (0 where empty), inst u8[n,H,W] (slot + 1, 0 where
    empty), face i32[n,H,W] (global face id, -1 where empty), px_all / px_vis i32[n,S], bbox_vis i32[n,S,4] = (xmin, ymin, xmax, ymax)
    of the visible pixels ((W, H, -1, -1) for none), visib_fract f32[n,S] = px_vis / px_all (0 for an empty slot).  No host
    synchronisation when the arguments are device tensors already; the call captures in a hipGraph."""
    from . import ops
    if scene.device is None:
        raise RuntimeError("this SceneMeshes was packed with device=None: render_frames has no CPU fallback (render_frames_numpy restates it)")
    dev = scene.device
    RT = torch.as_tensor(RT).to(device=dev, dtype=torch.float64)
    if RT.dim() != 4 or tuple(RT.shape[2:]) != (3, 4):
        raise ValueError("RT must be [n,S,3,4], got %s" % (tuple(RT.shape),))
    n = RT.shape[0]
    if not torch.is_tensor(slot_obj):
        so = np.asarray(slot_obj)
        if so.size and (so.min() < -1 or so.max() >= scene.n_objects):          # a host array can be looked at: refuse here
            raise ValueError("slot_obj holds an object outside [-1, %d)" % scene.n_objects)
    slot_obj = torch.as_tensor(slot_obj).to(device=dev, dtype=torch.int32)
    K = torch.as_tensor(K).to(device=dev, dtype=torch.float64)
    if light is None or not torch.is_tensor(light):
        light = torch.from_numpy(_light(light, n))
    light = light.to(device=dev, dtype=torch.float64).expand(n, 3).contiguous()
    textures = (scene.fuv, scene.tex, scene.tex_tab, scene.flip_v) if scene.has_texture else None
    rgb, depth, inst, face, stats = ops.render_frames(scene.verts, scene.vcol, scene.vnrm, scene.faces, scene.obj_face0, slot_obj,
                                                      RT.contiguous(), K.contiguous(), light, H, W, ambient, near, textures=textures)
    return _outputs(rgb, depth, inst, face, stats, torch)


def render_frames_numpy(scene, slot_obj, RT, K, H, W, light=None, ambient=AMBIENT, near=NEAR):
    """The rule of gdm_render_frames_hip (include/gdm.h) on the host, operation for operation in fp64: the dict of
    render_frames as numpy arrays (coverage and depth from pixel_rule.covered) plus `ambiguous` bool[n,H,W]: the pixels whose two best candidate depths, over all faces and
    slots, lie within 2 fp32 ulp of each other -- where the winner is not robust against the last bit of a division.  A scene with a
    texture is coloured by THE TEXTURE RULE (texture.py) where the winner's object has one, and then also returns `tex_level`
    i8[n,H,W]: the pyramid level every such pixel fetched from, -1 elsewhere."""
    from . import texture
    verts = scene.verts_np.astype(np.float64)
    vcol, vnrm = scene.vcol_np.astype(np.float64), scene.vnrm_np.astype(np.float64)
    faces, face0, O = scene.faces_np.astype(np.int64), scene.obj_face0, scene.n_objects
    slot_obj, RT = _np(slot_obj, np.int64), _np(RT, np.float64)
    n, S = slot_obj.shape
    K = np.broadcast_to(_np(K, np.float64), (n, 3, 3))
    light = _light(light, n)
    ambient = float(ambient)
    keys = np.full((n, S, H, W), _EMPTY, dtype=np.uint64)
    d1 = np.full((n, H, W), np.inf, dtype=np.float32)                      # the two best candidate depths of every pixel
    d2 = np.full((n, H, W), np.inf, dtype=np.float32)
    proj = {}
    for b in range(n):
        for s in range(S):
            o = int(slot_obj[b, s])
            if not 0 <= o < O:
                continue
            ok, xs, ys, iz = proj[b, s] = pixel_rule.project(verts, RT[b, s], K[b], near)
            for f, (px0, py0, px1, py1), inside, d in pixel_rule.covered(faces, ok, xs, ys, iz, H, W, face0[o], face0[o + 1]):
                tile = keys[b, s, py0:py1 + 1, px0:px1 + 1]
                tile[inside] = np.minimum(tile[inside], pixel_rule.depth_keys(d, f)[inside])
                t1, t2 = d1[b, py0:py1 + 1, px0:px1 + 1], d2[b, py0:py1 + 1, px0:px1 + 1]
                t2[inside] = np.minimum(t2[inside], np.maximum(t1[inside], d[inside]))
                t1[inside] = np.minimum(t1[inside], d[inside])
    bits = (keys >> np.uint64(32)).astype(np.int64)                        # [n,S,H,W]
    win = np.argmin(bits, axis=1)                                          # the first minimum: the lower slot on a tie
    best = np.take_along_axis(keys, win[:, None], axis=1)[:, 0]
    best_bits = (best >> np.uint64(32)).astype(np.int64)
    empty = best == _EMPTY
    inst = np.where(empty, 0, win + 1).astype(np.uint8)
    face = np.where(empty, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(empty, 0, best_bits).astype(np.uint32).view(np.float32)
    stats = np.zeros((n, S, 6), dtype=np.int32)
    rgb = np.zeros((n, H, W, 3), dtype=np.uint8)
    tex_level = np.full((n, H, W), -1, dtype=np.int8)
    for b in range(n):
        for s in range(S):
            rows, cols = np.nonzero(inst[b] == s + 1)
            stats[b, s] = ((keys[b, s] != _EMPTY).sum(), len(rows), cols.min() if len(rows) else W, rows.min() if len(rows) else H,
                           cols.max() if len(rows) else -1, rows.max() if len(rows) else -1)
            if not len(rows):
                continue
            _, xs, ys, iz = proj[b, s]
            i0, i1, i2 = faces[face[b, rows, cols]].T
            A2 = (xs[i1] - xs[i0]) * (ys[i2] - ys[i0]) - (xs[i2] - xs[i0]) * (ys[i1] - ys[i0])
            i1, i2 = np.where(A2 < 0, i2, i1), np.where(A2 < 0, i1, i2)   # the attributes follow the winding
            PX, PY = cols.astype(np.int64) * 256, rows.astype(np.int64) * 256
            q = []
            for a, c, opp in ((i1, i2, i0), (i2, i0, i1), (i0, i1, i2)):
                q.append(pixel_rule.edge(xs, ys, a, c, PX, PY).astype(np.float64) * iz[opp])
            Q = (q[0] + q[1]) + q[2]

            def interp(attr):
                return ((q[0] * attr[i0] + q[1] * attr[i1]) + q[2] * attr[i2]) / Q

            ox, oy, oz = interp(vnrm[:, 0]), interp(vnrm[:, 1]), interp(vnrm[:, 2])
            R = RT[b, s, :, :3]
            nx = (R[0, 0] * ox + R[0, 1] * oy) + R[0, 2] * oz
            ny = (R[1, 0] * ox + R[1, 1] * oy) + R[1, 2] * oz
            nz = (R[2, 0] * ox + R[2, 1] * oy) + R[2, 2] * oz
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)
            with np.errstate(all="ignore"):
                cs = np.where(length > 0, np.maximum(((nx * light[b, 0] + ny * light[b, 1]) + nz * light[b, 2]) / length, 0.0), 0.0)
            k = ambient + (1.0 - ambient) * cs
            row = scene.tex_tab_np[int(slot_obj[b, s])] if scene.has_texture else None
            if row is not None and texture.valid_row(row, len(scene.tex_np)):
                texel, tex_level[b, rows, cols] = _textured_levels(scene, row, q, Q, (i0, i1, i2), A2 < 0, face[b, rows, cols], xs, ys,
                                                                   iz, PX, PY)
                for ch in range(3):
                    rgb[b, rows, cols, ch] = np.minimum(255.0, np.floor(texel[:, ch].astype(np.float64) * k + 0.5)).astype(np.uint8)
                continue
            for ch in range(3):
                rgb[b, rows, cols, ch] = np.minimum(255.0, np.floor(interp(vcol[:, ch]) * k + 0.5)).astype(np.uint8)
    out = _outputs(rgb, depth, inst, face, stats, np)
    gap = d2.view(np.int32).astype(np.int64) - d1.view(np.int32).astype(np.int64)
    out["ambiguous"] = np.isfinite(d2) & (gap <= 2)
    if scene.has_texture:
        out["tex_level"] = tex_level
    return out


def _textured_levels(scene, row, q, Q, tri, swapped, fidx, xs, ys, iz, PX, PY):
    """The textured branch of the resolve pass for the pixels of one slot: q, Q the pixel's perspective weights, tri = (i0, i1, i2)
    with the winding's swap applied, swapped where it was, fidx the winning faces, (PX, PY) the pixels in 1/256 px -> the fetched
    colour levels u8[P,3] before shading, and the pyramid level i64[P] of each.  Operation for operation what resolve_kernel<VT, true> does."""
    from . import texture
    off, W0, H0, L = (int(x) for x in row)
    i0, i1, i2 = tri
    uv = scene.fuv_np.astype(np.float64)[fidx]                             # [P,3,2]: the corners follow the winding
    c0, c1, c2 = uv[:, 0], np.where(swapped[:, None], uv[:, 2], uv[:, 1]), np.where(swapped[:, None], uv[:, 1], uv[:, 2])

    def at(qq, QQ, ch):
        return ((qq[0] * c0[:, ch] + qq[1] * c1[:, ch]) + qq[2] * c2[:, ch]) / QQ

    u, v = at(q, Q, 0), at(q, Q, 1)
    fine, d = np.ones(len(u), dtype=bool), []
    with np.errstate(all="ignore"):
        for dx, dy in ((256, 0), (0, 256)):
            qn = [pixel_rule.edge(xs, ys, a, c, PX + dx, PY + dy).astype(np.float64) * iz[opp]
                  for a, c, opp in ((i1, i2, i0), (i2, i0, i1), (i0, i1, i2))]
            Qn = (qn[0] + qn[1]) + qn[2]
            fine &= Qn > 0.0
            d.append((at(qn, Qn, 0) * float(W0), at(qn, Qn, 1) * float(H0)))
        U, V = u * float(W0), v * float(H0)
        level = texture.mip_level_numpy(U, V, d[0][0], d[0][1], d[1][0], d[1][1], L, fine)
    out = np.zeros((len(u), 3), dtype=np.uint8)
    for l in np.unique(level):
        m = level == l
        out[m] = texture.fetch_numpy(scene.tex_np, H0, W0, int(l), u[m], v[m], scene.flip_v, offset=off)
    return out, level


# ---- built-in meshes ---------------------------------------------------------------------------------------------------------------
def _mix32(x):
    from .frontend import _mix32 as mix
    return mix(np.atleast_1d(np.asarray(x, dtype=np.uint32)))


def _uniform(seed, index, j):
    """Counter-based draws in [0, 1): word j of counter `index` (an array) under `seed`, 32 bits each, as float64."""
    base = _mix32(_mix32(np.uint32(seed & 0xFFFFFFFF) ^ np.uint32(0x9E3779B9)) ^ np.asarray(index, dtype=np.uint32))
    return _mix32(base ^ np.uint32(((j + 1) * 0x9E3779B9) & 0xFFFFFFFF)).astype(np.float64) / 4294967296.0


def demo_mesh(level=3, seed=0, textured=False, tex_size=64):
    """A bumpy subdivided icosahedron with hash-drawn vertex colours: 20 * 4**level faces, diameter about 0.1 (metres), no symmetry.
    The colours are drawn per vertex of the once-subdivided solid (42 of them) and averaged onto the finer vertices, so that they
    vary over the surface more slowly than the sampling does.  -> dict(verts f64[V,3], faces i32[F,3], normals f32[V,3], colors
    u8[V,3]), the mesh dict model_prep.build_model_points takes.  textured=True: the same solid as a textured object without any
    file -- colors None, uv f32[F,3,2] and texture u8[tex_size, 2 tex_size, 3] (_demo_texture)."""
    from . import model_prep
    level = int(level)
    if not 0 <= level <= 7:
        raise ValueError("level=%d not in [0, 7]" % level)
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [np.asarray(c, dtype=np.float64) / np.sqrt(1.0 + p * p) for c in
         ((-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1),
          (-p, 0, 1))]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    col = None
    for lv in range(level + 1):
        if lv == min(level, 1):                                            # the coarse vertices get their colours here
            idx = np.arange(len(v))
            col = [np.array([64.0 + 191.0 * _uniform(seed, idx[i:i + 1], ch)[0] for ch in range(3)]) for i in range(len(v))]
        if lv == level:
            break
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                if col is not None:
                    col.append(0.5 * (col[a] + col[b]))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    d = np.asarray(v)
    ph = 2.0 * np.pi * _uniform(seed, np.arange(6) + 1000, 3)
    bump = (1.0 + 0.12 * np.sin(3.0 * d[:, 0] + ph[0]) * np.cos(2.0 * d[:, 1] + ph[1]) + 0.08 * np.sin(5.0 * d[:, 2] + ph[2])
            + 0.10 * np.sin(2.0 * d[:, 0] + 3.0 * d[:, 1] + ph[3]))
    verts = d * bump[:, None] * np.array([0.05, 0.042, 0.034])
    faces = np.asarray(f, dtype=np.int32)
    normals = model_prep.vertex_normals_numpy(verts, faces).astype(np.float32)
    if textured:
        uv, image = _demo_texture(d, faces, seed, int(tex_size))
        return dict(verts=verts, faces=faces, normals=normals, colors=None, uv=uv, texture=image)
    return dict(verts=verts, faces=faces, normals=normals, colors=np.floor(np.asarray(col) + 0.5).astype(np.uint8))


def _demo_texture(d, faces, seed, size):
    """A seamed spherical parametrisation of the unit directions d f64[V,3] per face CORNER, and a hash-drawn image for it.  The
    longitude of a vertex is one number, so a face that straddles longitude +-pi gets 1 added at its corners on the low side: the seam
    lives in the corners and no vertex is doubled.  Fetches clamp to the edge and never wrap, so the longitude is mapped to u in [0, 1/2)
    (up to 3/4 on a seam face) and the image's right half repeats its left half.  v = colatitude / pi; a pole corner takes the mean u of
    the face's other corners.  The image: size x 2 size texels, a colour drawn per block of 4 x 4 texels plus a per-texel grain."""
    if size < 8 or size > 4096 or size % 4:
        raise ValueError("tex_size=%d must be a multiple of 4 in [8, 4096]" % size)
    lon = np.arctan2(d[:, 1], d[:, 0]) / (2.0 * np.pi) + 0.5               # [0, 1]
    lat = np.arccos(np.clip(d[:, 2], -1.0, 1.0)) / np.pi
    pole = np.abs(d[:, 2]) > 1.0 - 1e-12
    fu, fv, fp = lon[faces], lat[faces], pole[faces]                       # [F,3]
    span = np.where(fp, np.nan, fu)
    wrap = (np.nanmax(span, axis=1) - np.nanmin(span, axis=1)) > 0.5
    fu = np.where(wrap[:, None] & (fu < 0.5), fu + 1.0, fu)
    mean = np.nanmean(np.where(fp, np.nan, fu), axis=1)
    fu = np.where(fp, mean[:, None], fu)
    uv = np.stack([fu * 0.5, fv], axis=-1).astype(np.float32)
    by, bx = np.meshgrid(np.arange(size) // 4, np.arange(size) // 4, indexing="ij")
    ty, tx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    half = np.stack([np.floor(40.0 + 150.0 * _uniform(seed, (by * 1024 + bx).ravel() + 20000, ch)
                              + 60.0 * _uniform(seed, (ty * 4096 + tx).ravel() + 9000000, ch)).reshape(size, size) for ch in range(3)], axis=-1)
    return uv, np.ascontiguousarray(np.concatenate([half, half], axis=1).astype(np.uint8))


def backdrop_mesh(K, H, W, z=1.5, grid=(4, 3), margin=8.0, seed=0):
    """A plane at depth z of the camera frame (pose it with the identity) that covers the H x W image of K and `margin` pixels round
    it, as a grid of grid[0] x grid[1] cells of two triangles with hash-drawn vertex colours; its normals face the camera."""
    K = _np(K, np.float64).reshape(-1, 3, 3)[0]
    gx, gy = int(grid[0]), int(grid[1])
    if gx < 1 or gy < 1:
        raise ValueError("grid=%r must hold at least one cell each way" % (grid,))
    us = np.linspace(-margin, W - 1 + margin, gx + 1)
    vs = np.linspace(-margin, H - 1 + margin, gy + 1)
    U, V = np.meshgrid(us, vs)
    verts = np.stack([(U - K[0, 2]) / K[0, 0] * z, (V - K[1, 2]) / K[1, 1] * z, np.full(U.shape, float(z))], axis=-1).reshape(-1, 3)
    faces = []
    for j in range(gy):
        for i in range(gx):
            a = j * (gx + 1) + i
            faces += [(a, a + 1, a + gx + 2), (a, a + gx + 2, a + gx + 1)]
    idx = np.arange(len(verts)) + 5000
    colors = np.stack([np.floor(32.0 + 192.0 * _uniform(seed, idx, ch)) for ch in range(3)], axis=1).astype(np.uint8)
    normals = np.tile(np.array([0.0, 0.0, -1.0], dtype=np.float32), (len(verts), 1))
    return dict(verts=verts, faces=np.asarray(faces, dtype=np.int32), normals=normals, colors=colors)


# ---- poses ---------------------------------------------------------------------------------------------------------------------------
def _rotation(u1, u2, u3):
    """A rotation matrix from three uniforms (Shoemake's uniform unit quaternion)."""
    a, b = np.sqrt(1.0 - u1), np.sqrt(u1)
    x, y, z, w = a * np.sin(2 * np.pi * u2), a * np.cos(2 * np.pi * u2), b * np.sin(2 * np.pi * u3), b * np.cos(2 * np.pi * u3)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sample_scene_poses(n, S, seed, K, H, W, z_range=(0.4, 1.0), target_obj=0, distractor_objs=(0,), backdrop_obj=None, radius=0.05,
                       occlude_prob=0.5, margin=0.15, first=0):
    """Poses of n frames of S slots, on the host (a few hundred doubles per batch), from counter-based draws (lowbias32 of (seed,
    frame, slot, word): frame first + b of a seed is the same whatever the batch it comes in) -> slot_obj i32[n,S], RT f64[n,S,3,4].
    Slot 0 is `target_obj`, its centre projecting inside the image (`margin`: the share of each side kept free) at a depth in z_range.
    The last slot is `backdrop_obj` under the identity when given.  Every other slot holds one of `distractor_objs` (empty when the
    tuple is): with probability occlude_prob in FRONT of the target -- 1.5 to 3 `radius` nearer, 0.6 to 1.6 radius aside, so that it
    covers a part of it --, otherwise anywhere in the image at a depth in z_range."""
    K = _np(K, np.float64).reshape(-1, 3, 3)[0]
    n, S = int(n), int(S)
    if n < 1 or not 1 <= S <= 8:
        raise ValueError("n=%d must be positive and S=%d in [1, 8]" % (n, S))
    slot_obj = np.full((n, S), -1, dtype=np.int32)
    RT = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (n, S, 1, 1))
    z0, z1 = float(z_range[0]), float(z_range[1])

    def back(u, v, z):
        return np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])

    for b in range(n):
        for s in range(S):
            d = [float(_uniform(seed, [((first + b) * 8 + s) & 0xFFFFFFFF], j)[0]) for j in range(9)]
            R = _rotation(d[0], d[1], d[2])
            if s == 0:
                slot_obj[b, s] = target_obj
                t = back((margin + (1 - 2 * margin) * d[3]) * (W - 1), (margin + (1 - 2 * margin) * d[4]) * (H - 1), z0 + (z1 - z0) * d[5])
            elif backdrop_obj is not None and s == S - 1:
                slot_obj[b, s] = backdrop_obj
                continue
            elif len(distractor_objs):
                slot_obj[b, s] = distractor_objs[int(d[6] * len(distractor_objs)) % len(distractor_objs)]
                if d[7] < occlude_prob:
                    tt = RT[b, 0, :, 3]
                    ang, off = 2 * np.pi * d[3], (0.6 + 1.0 * d[4]) * radius
                    zf = max(tt[2] - (1.5 + 1.5 * d[5]) * radius, 0.5 * z0)        # on the target's line of sight, then aside
                    t = tt * (zf / tt[2]) + np.array([off * np.cos(ang), off * np.sin(ang), 0.0])
                else:
                    t = back(d[3] * (W - 1), d[4] * (H - 1), z0 + (z1 - z0) * d[5])
            else:
                continue
            RT[b, s] = np.hstack([R, t[:, None]])
    return slot_obj, RT


# ---- training batches ------------------------------------------------------------------------------------------------------------------
class RenderedFrames:
    """An iterable of `n_batches` training batches of `batch` rendered items of object `target_obj` of `scene` (metres):
      1. sample_scene_poses(batch, S, seed, ...) for frames first, first + 1, ... of the seed, and render_frames;
      2. mask = (inst == 1) * 255, bbox = bbox_vis[:, 0];
      3. frontend.make_inputs_from_boxes(rgb, depth, K, bbox, S_crop, n_points, mask=mask, train=True, sampler="hash", jitter="hash",
         seed=...) -- crop, normals, hash sampling and the pyramid;
      4. + RT (slot 0, f32[B,3,4]), K, cls_id, px_vis and visib_fract of the target.
    labels, match_idx and visible_flag are train_lm.device_targets' (--gt-targets device).  An item whose target shows fewer than
    min_px_vis pixels or whose crop holds fewer than min_valid depth pixels (the loader's 200, linemod_pbr.py:479) gets
    origin_labels = 0 on the device, which is what device_targets replaces by the batch's first valid item: no host read.
    model_xyz f32[M,3] (metres) gives the radius the distractors are placed by.  train=False (held-out frames for -state=test):
    no box jitter, and the batch carries scene_id / im_id.  build_pyramid=False leaves the neighbour pyramid (which wants n_points >=
    1024) to the consumer, as make_inputs_from_boxes does.  keep_frames=True: a batch also carries frame_depth f32[B,H,W] (the rendered
    depth frame) and bbox f32[B,4] (the target's visible box), what pose.verify_poses wants; the default leaves the batch as it is.
    depth_sensor: a sensor.DepthSensor, or None (the default: every tensor of the batch is what it was without the argument).  With one,
    the rendered depth passes through sensor.simulate_depth_sensor (seed sensor_seed(i)) before make_inputs_from_boxes, so the crop, its
    normals and cld_rgb_nrm are a camera's; the mask, the box, RT and the statistics stay the renderer's.  With keep_frames the batch's
    frame_depth is then the SENSED frame, and it also carries frame_depth_clean f32[B,H,W] and depth_cause u8[B,H,W]."""

    def __init__(self, scene, target_obj, model_xyz, batch, n_points, S_crop=256, seed=0, n_batches=64, K=None, H=480, W=640, S=4,
                 z_range=(0.4, 1.0), distractor_objs=None, backdrop_obj=None, min_px_vis=64, min_valid=200, train=True, cls_id=None,
                 light=None, ambient=AMBIENT, near=NEAR, build_pyramid=True, keep_frames=False, depth_sensor=None):
        from . import synthetic
        self.scene, self.target_obj, self.batch, self.n_points, self.S_crop = scene, int(target_obj), int(batch), int(n_points), int(S_crop)
        self.seed, self.n_batches, self.H, self.W, self.S = int(seed), int(n_batches), int(H), int(W), int(S)
        self.K = _np(synthetic.LM_K if K is None else K, np.float64)
        xyz = _np(model_xyz, np.float64)
        self.radius = float(np.linalg.norm(xyz - xyz.mean(0), axis=1).max())
        self.z_range, self.backdrop_obj = z_range, backdrop_obj
        others = [o for o in range(scene.n_objects) if o != backdrop_obj]
        self.distractor_objs = tuple(others if distractor_objs is None else distractor_objs)
        self.min_px_vis, self.min_valid, self.train, self.cls_id = int(min_px_vis), int(min_valid), bool(train), cls_id
        self.light, self.ambient, self.near, self.build_pyramid = light, ambient, near, bool(build_pyramid)
        self.keep_frames = bool(keep_frames)
        self.depth_sensor = depth_sensor
        dev = scene.device
        self._K32 = torch.from_numpy(self.K.astype(np.float32)).to(dev).expand(self.batch, 3, 3).contiguous()
        self._K64 = torch.from_numpy(self.K).to(dev)

    def __len__(self):
        return self.n_batches

    def frames(self, i):
        """The poses and the rendered frames of batch i: (slot_obj, RT f64[B,S,3,4] on the host, the dict of render_frames)."""
        slot_obj, RT = sample_scene_poses(self.batch, self.S, self.seed, self.K, self.H, self.W, self.z_range, self.target_obj,
                                          self.distractor_objs, self.backdrop_obj, self.radius, first=i * self.batch)
        return slot_obj, RT, render_frames(self.scene, slot_obj, RT, self._K64, self.H, self.W, self.light, self.ambient, self.near)

    def item_seed(self, i):
        return (self.seed * 1000003 + i * 7919 + 1) & 0x7FFFFFFF

    def sensor_seed(self, i):
        """The seed of batch i's depth sensor call, derived from its item seed."""
        return (self.item_seed(i) ^ 0x5BD1E995) & 0xFFFFFFFF

    def batch_at(self, i):
        from . import frontend
        _, RT, fr = self.frames(i)
        dev = self.scene.device
        mask = (fr["inst"] == 1).to(torch.uint8) * 255
        bbox = fr["bbox_vis"][:, 0].to(torch.float32)
        item_seed = self.item_seed(i)
        depth, sensed = fr["depth"], None
        if self.depth_sensor is not None:
            from . import sensor
            sensed = sensor.simulate_depth_sensor(depth, self.K.astype(np.float32), self.depth_sensor, seed=self.sensor_seed(i))
            depth = sensed["depth"]
        item = frontend.make_inputs_from_boxes(fr["rgb"], depth, self._K32, bbox, self.S_crop, self.n_points, mask=mask,
                                               train=self.train, sampler="hash", jitter="hash", seed=item_seed,
                                               build_pyramid=self.build_pyramid)
        keep = (fr["px_vis"][:, 0] >= self.min_px_vis) & (item["n_valid"] >= self.min_valid)
        labels = item["origin_labels"].to(torch.int32)                      # the loader's dtype
        item["origin_labels"] = torch.where(keep[:, None], labels, torch.zeros_like(labels))
        item["RT"] = torch.from_numpy(RT[:, 0].astype(np.float32)).to(dev)
        item["K"] = self._K32
        item["px_vis"], item["visib_fract"] = fr["px_vis"][:, 0].contiguous(), fr["visib_fract"][:, 0].contiguous()
        if self.cls_id is not None:
            item["cls_id"] = torch.full((self.batch,), int(self.cls_id), dtype=torch.int32, device=dev)
        if not self.train:
            item["scene_id"] = torch.full((self.batch,), 1 + self.seed, dtype=torch.int32)
            item["im_id"] = torch.arange(i * self.batch, (i + 1) * self.batch, dtype=torch.int32)
        if self.keep_frames:
            item["frame_depth"], item["bbox"] = depth, bbox
            if sensed is not None:
                item["frame_depth_clean"], item["depth_cause"] = fr["depth"], sensed["cause"]
        return item

    def __iter__(self):
        for i in range(self.n_batches):
            yield self.batch_at(i)
