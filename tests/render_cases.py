"""The fixture scenes shared by tests/test_render_frames_cpu.py and tests/test_gpu_frames_render.py: the squashed icosphere and the
61 x 45 camera of tests/golden/bop_inputs.py, posed as scenes for render.render_frames.  Pure numpy, seeded."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import bop_inputs as bi  # noqa: E402

H, W, NEAR, AMBIENT = bi.H, bi.W, bi.NEAR, 0.3


def colours(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 3)).astype(np.uint8)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def pose(R, t):
    return np.hstack([R, np.asarray(t, dtype=np.float64)[:, None]])


def fixture_mesh(seed=1, scale=1.0):
    """(verts, faces, colours, None): the normals are left to SceneMeshes."""
    v, f = bi.mesh()
    return (v * scale, f, colours(len(v), seed), None)


def quad_mesh(z=0.5, colour=None, seed=3):
    v, f = bi.full_quad(z=z)
    c = colours(4, seed) if colour is None else np.tile(np.asarray(colour, dtype=np.uint8), (4, 1))
    return (v, f, c, np.tile(np.array([0.0, 0.0, -1.0], dtype=np.float32), (4, 1)))


def two_objects():
    """The fixture mesh twice (the second copy at half size) as two objects and a backdrop quad at z = 0.5: S = 3, n = 3, K per
    instance.  Object 0 stands at z = 0.35-0.38 (bop_inputs.poses()' estimates: near, far, clipped), object 1 in front of it at
    z = 0.18; the meshes reach 0.08 and 0.04 from their centres, so it occludes a part of object 0 without ever coming within 4 cm
    of it.  Frame 1 leaves object 1's slot empty."""
    est, _ = bi.poses()
    RT = np.zeros((3, 3, 3, 4))
    RT[:, 0] = est
    for b, (ang, axis, t) in enumerate([(0.9, (0, 1, 1), (0.02, 0.0, 0.18)), (0.3, (1, 0, 0), (0.0, 0.0, 0.18)),
                                        (2.1, (1, 1, 0), (0.07, 0.01, 0.18))]):
        RT[b, 1] = pose(bi.rot(ang, axis), t)
    RT[:, 2] = bi.identity_pose()[0]
    slot_obj = np.array([[0, 1, 2], [0, -1, 2], [0, 1, 2]], dtype=np.int32)
    K = np.stack([bi.K, bi.K + np.array([[3.0, 0, 1.5], [0, -2.0, -0.75], [0, 0, 0]]), bi.K])
    light = np.stack([unit((0.3, -0.2, -1.0)), unit((0, 0, -1.0)), unit((-0.5, 0.4, -0.6))])
    return dict(meshes=[fixture_mesh(1), fixture_mesh(2, 0.5), quad_mesh(0.5)], slot_obj=slot_obj, RT=RT, K=K, light=light)


def tilted_quad():
    """The full-image quad tilted about (1, 1, 0): two triangles far larger than the per-thread limit, depth varying over them."""
    RT = pose(bi.rot(0.5, (1, 1, 0)), (0.0, 0.0, 0.25))[None, None]
    return dict(meshes=[quad_mesh(0.5)], slot_obj=np.zeros((1, 1), dtype=np.int32), RT=RT, K=bi.K, light=unit((0.2, 0.1, -1.0))[None])


def tilted_quad_twice():
    """The tilted quad in slots 0 and 1 of one frame, the second 0.1 farther along z: four large triangles of two slots in one wave."""
    RT = np.stack([pose(bi.rot(0.5, (1, 1, 0)), (0.0, 0.0, 0.25 + 0.1 * s)) for s in range(2)])[None]
    return dict(meshes=[quad_mesh(0.5)], slot_obj=np.zeros((1, 2), dtype=np.int32), RT=RT, K=bi.K, light=unit((0.2, 0.1, -1.0))[None])


SCENES = {"two objects": two_objects, "tilted quad": tilted_quad, "tilted quad twice": tilted_quad_twice}          # the scenes the GPU file compares with the restatement


def render_args(case):
    """(slot_obj, RT, K, H, W) and the keywords of render_frames / render_frames_numpy for a scene dict."""
    return (case["slot_obj"], case["RT"], case["K"], H, W), dict(light=case["light"], ambient=AMBIENT, near=NEAR)
