"""CPU: the three host restatements that draw with pixel_rule (evaluation.render_depth_numpy, pose.raster_depth_face_numpy and a
one-slot render.render_frames_numpy) give the same depth bits and the same faces, and a face whose index lies outside [0, V) is
discarded by all three, as tri_setup of csrc/gdm_raster.h discards it."""
import numpy as np

import verify_cases as vc
from geometric_aware_dense_matching_amd import evaluation, pose, render


def _three(verts, faces, rt):
    """depth f32[H,W] (0 where nothing is drawn) and face i64[H,W] (-1 there) of each restatement that keeps them."""
    d_eval = evaluation.render_depth_numpy(verts, faces, rt[None], vc.K0, vc.H, vc.W, vc.NEAR)[0]
    z, f_pose = pose.raster_depth_face_numpy(verts, faces, rt, vc.K0, vc.H, vc.W, vc.NEAR)
    d_pose = np.where(np.isinf(z), np.float32(0), z)
    scene = render.SceneMeshes([(verts, np.zeros((1, 3), dtype=np.int64))], device=None, verts_dtype=verts.dtype)
    scene.faces_np = np.ascontiguousarray(faces.astype(np.int32))          # SceneMeshes itself refuses an index outside [0, V)
    scene.obj_face0 = [0, len(faces)]
    out = render.render_frames_numpy(scene, [[0]], rt[None, None], vc.K0, vc.H, vc.W, near=vc.NEAR)
    return (d_eval, None), (d_pose, f_pose), (out["depth"][0], out["face"][0].astype(np.int64))


def _assert_agree(images):
    (d0, _), (d1, f1), (d2, f2) = images
    assert d0.dtype == d1.dtype == d2.dtype == np.float32
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(d0.view(np.uint32), d2.view(np.uint32))
    assert np.array_equal(f1, f2) and np.array_equal(f1 >= 0, d0 > 0)


def test_the_three_restatements_agree_bit_for_bit():
    verts, faces = vc.mixed_mesh(2)
    assert len(faces) == 323
    rt = vc._candidates(1, 1, seed=20)[0, 0]
    images = _three(verts.astype(np.float32), faces, rt)
    _assert_agree(images)
    d, f = images[1]
    assert (f == 320).sum() > vc.H * vc.W // 2                            # the large triangle, face 320, wins most of the frame


def test_a_face_index_outside_the_vertices_is_discarded():
    verts, faces = vc.mixed_mesh(1)
    verts = verts.astype(np.float32)
    V = len(verts)
    bad = np.concatenate([[[0, 1, -1]], faces[:40], [[V, 2, 3]], faces[40:]]).astype(np.int32)
    rt = vc._candidates(1, 1, seed=20)[0, 0]
    clean, dirty = _three(verts, faces, rt), _three(verts, bad, rt)
    _assert_agree(dirty)
    renumber = np.concatenate([np.arange(40) + 1, np.arange(40, len(faces)) + 2])
    for (dc, fc), (dd, fd) in zip(clean, dirty):
        assert np.array_equal(dc.view(np.uint32), dd.view(np.uint32))
        if fc is not None:
            assert np.array_equal(np.where(fc >= 0, renumber[np.maximum(fc, 0)], -1), fd)
