"""What tests/test_texture_cpu.py and tests/test_gpu_frames_textured.py share: a PLY writer that knows the three places a texture
coordinate can live, hash-drawn images, and the textured scene of the GPU comparison.  Pure numpy, seeded."""
import numpy as np

from geometric_aware_dense_matching_amd import render

NEAR, AMBIENT = 0.01, 0.3


def image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def write_ply(path, verts, faces, binary, vertex_uv=None, uv_names=("texture_u", "texture_v"), face_uv=None, texture_file=None):
    """verts f32[V,3], faces i32[F,3]; vertex_uv f32[V,2] under the property names uv_names; face_uv: a list of F sequences of floats,
    written as the face list property `texcoord` after an int scalar `texnumber` (MeshLab's layout) -- ragged when the lengths differ."""
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment made by a test"]
    if texture_file:
        head.append("comment TextureFile %s" % texture_file)
    head += ["element vertex %d" % len(verts), "property float x", "property float y", "property float z"]
    if vertex_uv is not None:
        head += ["property float %s" % uv_names[0], "property float %s" % uv_names[1]]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices"]
    if face_uv is not None:
        head += ["property list uchar float texcoord", "property int texnumber"]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for k, v in enumerate(verts):
            row = [float(x) for x in v] + ([float(x) for x in vertex_uv[k]] if vertex_uv is not None else [])
            f.write(np.asarray(row, dtype="<f4").tobytes() if binary else (" ".join(repr(x) for x in row) + "\n").encode())
        for k, t in enumerate(faces):
            if binary:
                f.write(np.uint8(3).tobytes() + np.asarray(t, dtype="<i4").tobytes())
                if face_uv is not None:
                    f.write(np.uint8(len(face_uv[k])).tobytes() + np.asarray(face_uv[k], dtype="<f4").tobytes() + np.int32(0).tobytes())
            else:
                row = "3 %d %d %d" % tuple(int(i) for i in t)
                if face_uv is not None:
                    row += " %d %s 0" % (len(face_uv[k]), " ".join(repr(float(x)) for x in face_uv[k]))
                f.write((row + "\n").encode())


def tetrahedron():
    verts = np.array([[0, 0, 0], [1.5, 0, 0], [0, -2.25, 0], [0, 0, 3.125], [4, 5, 6]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 4, 3]], dtype=np.int32)
    return verts, faces


def rot(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def pose(R, t):
    return np.hstack([R, np.asarray(t, dtype=np.float64)[:, None]])


# (H, W) of the frame and (th, tw) of the texture: the two sizes the textured comparison runs at
SIZES = [((48, 64), (16, 16)), ((37, 53), (33, 20))]


def textured_scene(frame, tex, k_per_instance):
    """n = 2 frames, S = 3 slots, O = 3 objects: the 320-face demo icosphere with a (th, tw) hash image as its texture (object 0), a
    vertex-coloured icosphere (object 1) and a backdrop plane (object 2).
      frame 0   object 0 FAR (about 3 px across: level >= 2), object 1 beside it, the backdrop
      frame 1   object 0 NEAR (about two thirds of the frame: magnified, level 0), object 0 again at the frame's edge, turned and
                pushed half out of the image (its limb is seen at a grazing angle: levels above the centre's), the backdrop
    -> dict(meshes, slot_obj, RT, K, light, H, W)."""
    (H, W), (th, tw) = frame, tex
    f = 60.0 * W / 64.0
    K0 = np.array([[f, 0, W / 2.0 - 0.5], [0, f * 1.02, H / 2.0 - 0.25], [0, 0, 1]])
    m = render.demo_mesh(level=2, seed=3, textured=True, tex_size=16)
    meshes = [(m["verts"], m["faces"], None, m["normals"], m["uv"], image(th, tw, 11)),
              render._as_mesh(render.demo_mesh(level=2, seed=4)), render._as_mesh(render.backdrop_mesh(K0, H, W, z=3.0))]
    eye = pose(np.eye(3), (0, 0, 0))
    RT = np.stack([np.stack([pose(rot(0.4, (1, 2, 0)), (0.03, -0.02, 2.0)), pose(rot(1.1, (0, 1, 1)), (-0.06, 0.01, 0.5)), eye]),
                   np.stack([pose(rot(2.0, (1, 0, 1)), (-0.01, 0.0, 0.13)), pose(rot(0.7, (0, 1, 0)), (0.115, 0.04, 0.22)), eye])])
    slot_obj = np.array([[0, 1, 2], [0, 0, 2]], dtype=np.int32)
    K = np.stack([K0, K0 + np.array([[2.0, 0, 0.75], [0, -1.5, -0.5], [0, 0, 0]])]) if k_per_instance else K0
    light = np.stack([np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0]), np.array([0.0, 0.0, -1.0])])
    return dict(meshes=meshes, slot_obj=slot_obj, RT=RT, K=K, light=light, H=H, W=W)


def render_args(case):
    return (case["slot_obj"], case["RT"], case["K"], case["H"], case["W"]), dict(light=case["light"], ambient=AMBIENT, near=NEAR)
