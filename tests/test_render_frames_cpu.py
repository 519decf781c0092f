"""CPU: render.render_frames_numpy, the host restatement of the frame renderer's written rule (include/gdm.h), alone:
its depth against evaluation.render_depth_numpy, hand-computed scenes, the windings, empty slots, the pose sampler, and the
precondition of the GPU comparison (no pixel of a fixture scene is decided by less than 2 ulp of depth)."""
import numpy as np
import pytest

import render_cases as rc
from render_cases import bi
from geometric_aware_dense_matching_amd import evaluation as ev
from geometric_aware_dense_matching_amd import render

H, W = rc.H, rc.W


def _scene(meshes, dtype=np.float64):
    return render.SceneMeshes(meshes, device=None, verts_dtype=dtype)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("which", ["est", "gt"])
def test_one_slot_depth_is_render_depth_numpy_bit_for_bit(which):
    verts, faces = bi.mesh()
    est, gt = bi.poses()
    RT = est if which == "est" else gt[:1]
    out = render.render_frames_numpy(_scene([(verts, faces)]), np.zeros((len(RT), 1), dtype=np.int32), RT[:, None], bi.K, H, W, near=bi.NEAR)
    want = ev.render_depth_numpy(verts, faces, RT, bi.K, H, W, bi.NEAR)
    assert out["depth"].dtype == np.float32 and np.array_equal(_bits(out["depth"]), _bits(want))
    assert np.array_equal(out["inst"] > 0, want > 0) and np.array_equal(out["face"] >= 0, want > 0)
    assert np.array_equal(out["px_all"][:, 0], (want > 0).reshape(len(RT), -1).sum(1)) and np.array_equal(out["px_vis"], out["px_all"])
    assert not out["rgb"][want == 0].any()
    assert not out["ambiguous"].any()


def test_full_image_quad_of_one_colour():
    colour, light, ambient = (200, 100, 31), rc.unit((0.0, 0.6, -0.8)), 0.25
    out = render.render_frames_numpy(_scene([rc.quad_mesh(0.5, colour)]), [[0]], bi.identity_pose()[:, None], bi.K, H, W, light=light,
                                     ambient=ambient, near=bi.NEAR)
    assert (out["depth"] == np.float32(0.5)).all() and (out["inst"] == 1).all() and (out["face"] >= 0).all()
    k = ambient + (1.0 - ambient) * 0.8                                    # the normal (0, 0, -1) against the light: cos = 0.8
    for ch in range(3):
        got = np.unique(out["rgb"][..., ch])
        want = np.floor(colour[ch] * k + 0.5)
        # the interpolation of three equal levels may leave the level by an ulp, which moves the result only at a rounding boundary
        assert len(got) == 1 and got[0] == want and abs(colour[ch] * k + 0.5 - np.round(colour[ch] * k + 0.5)) > 1e-6
    assert out["px_all"].tolist() == [[H * W]] and out["px_vis"].tolist() == [[H * W]]
    assert out["bbox_vis"].tolist() == [[[0, 0, W - 1, H - 1]]] and out["visib_fract"].tolist() == [[1.0]]


def _half_quad(z, u_max):
    """A fronto-parallel quad at depth z covering the pixel columns 0 .. u_max (its right edge at u_max + 0.5) and every row."""
    def back(u, v):
        return [(u - bi.K[0, 2]) / bi.K[0, 0] * z, (v - bi.K[1, 2]) / bi.K[1, 1] * z, z]
    verts = np.array([back(-2, -2), back(u_max + 0.5, -2), back(u_max + 0.5, H + 1), back(-2, H + 1)])
    return (verts, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), np.tile(np.uint8([10, 250, 90]), (4, 1)), None)


def test_two_occluding_quads_by_hand():
    near_cols = 30                                                         # the nearer quad covers columns 0..29
    scene = _scene([rc.quad_mesh(0.5, (255, 255, 255)), _half_quad(0.3, near_cols - 1)])
    RT = np.tile(bi.identity_pose()[:, None], (1, 2, 1, 1))
    out = render.render_frames_numpy(scene, [[0, 1]], RT, bi.K, H, W, near=bi.NEAR)
    want_inst = np.ones((H, W), dtype=np.uint8)
    want_inst[:, :near_cols] = 2
    assert np.array_equal(out["inst"][0], want_inst)
    assert out["px_all"].tolist() == [[H * W, H * near_cols]] and out["px_vis"].tolist() == [[H * (W - near_cols), H * near_cols]]
    assert np.array_equal(out["visib_fract"], np.float32([[np.float32(H * (W - near_cols)) / np.float32(H * W), 1.0]]))
    assert out["bbox_vis"].tolist() == [[[near_cols, 0, W - 1, H - 1], [0, 0, near_cols - 1, H - 1]]]
    assert (out["depth"][0, :, :near_cols] == np.float32(0.3)).all() and (out["depth"][0, :, near_cols:] == np.float32(0.5)).all()
    assert (out["face"][0, :, :near_cols] >= 2).all() and (out["face"][0, :, near_cols:] < 2).all()          # global face ids
    # the slots the other way round: the nearer object still wins, the slot numbers swap
    flipped = render.render_frames_numpy(scene, [[1, 0]], RT, bi.K, H, W, near=bi.NEAR)
    assert np.array_equal(flipped["inst"][0], 3 - want_inst) and np.array_equal(flipped["rgb"], out["rgb"])
    assert np.array_equal(flipped["face"], out["face"])


def test_flipped_windings_leave_the_images_unchanged():
    case = rc.two_objects()
    args, kw = rc.render_args(case)
    want = render.render_frames_numpy(_scene(case["meshes"]), *args, **kw)
    flipped = []
    for k, (v, f, c, nr) in enumerate(case["meshes"]):
        f = f.copy()
        f[k::2] = f[k::2][:, [0, 2, 1]]                                    # every other face the other way round
        nr = render.SceneMeshes([case["meshes"][k]], device=None).vnrm_np if nr is None else nr          # the normals stay the mesh's
        flipped.append((v, f, c, nr))
    got = render.render_frames_numpy(_scene(flipped), *args, **kw)
    for key in ("rgb", "depth", "inst", "face", "px_all", "px_vis", "bbox_vis", "visib_fract"):
        assert np.array_equal(got[key], want[key]), key


def test_empty_slot_and_object_out_of_view():
    verts, faces = bi.mesh()
    scene = _scene([(verts, faces)])
    RT = np.stack([rc.pose(np.eye(3), (0.0, 0.0, 0.35)), rc.pose(np.eye(3), (5.0, 0.0, 0.35)), rc.pose(np.eye(3), (0.0, 0.0, -0.35)),
                   rc.pose(np.eye(3), (0.0, 0.0, 0.35))])[None]
    out = render.render_frames_numpy(scene, [[0, 0, 0, -1]], RT, bi.K, H, W, near=bi.NEAR)
    stats = np.concatenate([out["px_all"][..., None], out["px_vis"][..., None], out["bbox_vis"]], axis=-1)[0]
    assert stats[0, 0] > 100 and stats[0, 1] == stats[0, 0]
    for s in (1, 2, 3):                                                    # beside the image, behind the camera, empty
        assert stats[s].tolist() == [0, 0, W, H, -1, -1], s
    assert out["visib_fract"][0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert set(np.unique(out["inst"]).tolist()) == {0, 1}
    # an object index outside the table is an empty slot too (the kernel never indexes with it)
    bad = render.render_frames_numpy(scene, [[0, 7, -3, -1]], RT, bi.K, H, W, near=bi.NEAR)
    assert np.array_equal(bad["inst"], out["inst"]) and np.array_equal(bad["px_all"], out["px_all"])


def test_pose_sampling_is_reproducible_and_keeps_the_target_inside():
    K = bi.LM_K
    kw = dict(z_range=(0.4, 1.0), target_obj=1, distractor_objs=(0, 1), backdrop_obj=2, radius=0.05)
    so, RT = render.sample_scene_poses(16, 4, 5, K, 480, 640, **kw)
    so2, RT2 = render.sample_scene_poses(16, 4, 5, K, 480, 640, **kw)
    assert so.dtype == np.int32 and so.shape == (16, 4) and RT.shape == (16, 4, 3, 4) and RT.dtype == np.float64
    assert np.array_equal(so, so2) and np.array_equal(RT, RT2)
    tail = render.sample_scene_poses(8, 4, 5, K, 480, 640, first=8, **kw)  # frame b of a seed does not depend on the batch it is in
    assert np.array_equal(tail[0], so[8:]) and np.array_equal(tail[1], RT[8:])
    other = render.sample_scene_poses(16, 4, 6, K, 480, 640, **kw)
    assert not np.array_equal(other[1], RT)
    assert (so[:, 0] == 1).all() and (so[:, 3] == 2).all() and set(so[:, 1:3].ravel().tolist()) <= {0, 1}
    t = RT[:, 0, :, 3]
    u, v = K[0, 0] * t[:, 0] / t[:, 2] + K[0, 2], K[1, 1] * t[:, 1] / t[:, 2] + K[1, 2]
    assert (u >= 0).all() and (u <= 639).all() and (v >= 0).all() and (v <= 479).all()
    assert (t[:, 2] >= 0.4).all() and (t[:, 2] <= 1.0).all()
    R = RT[:, :3, :, :3].reshape(-1, 3, 3)
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(R), 1.0)
    front = (RT[:, 1:3, 2, 3] < t[:, None, 2]).mean()
    assert 0.2 < front < 0.9                                               # some distractors stand in front of the target
    assert np.array_equal(RT[:, 3], np.tile(bi.identity_pose(), (16, 1, 1)))


def test_demo_and_backdrop_meshes():
    for level in (0, 2, 3):
        m = render.demo_mesh(level=level, seed=0)
        assert m["faces"].shape == (20 * 4 ** level, 3) and m["faces"].dtype == np.int32
        assert m["colors"].dtype == np.uint8 and m["normals"].dtype == np.float32 and m["verts"].shape == m["normals"].shape
    d = bi.diameter(m["verts"])
    assert 0.08 < d < 0.125
    assert (np.einsum("ij,ij->i", m["normals"], m["verts"]) > 0).all()     # outward normals
    again = render.demo_mesh(level=3, seed=0)
    assert np.array_equal(again["verts"], m["verts"]) and np.array_equal(again["colors"], m["colors"])
    assert not np.array_equal(render.demo_mesh(level=3, seed=1)["colors"], m["colors"])
    b = render.backdrop_mesh(bi.K, H, W, z=0.6, grid=(3, 2))
    out = render.render_frames_numpy(_scene([render._as_mesh(b)]), [[0]], bi.identity_pose()[:, None], bi.K, H, W, near=bi.NEAR)
    assert (out["inst"] == 1).all() and (np.abs(out["depth"] - 0.6) < 1e-6).all() and len(np.unique(out["rgb"])) > 10


@pytest.mark.parametrize("name", sorted(rc.SCENES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_fixture_pixel_is_decided_by_two_ulp_of_depth(name, dtype):
    """The precondition of the GPU comparison: where the two best candidate depths of a pixel lie within 2 ulp, a division that differs
    in its last bit could change `face` or `inst`; the fixture scenes hold no such pixel, for f64 and for f32 vertices."""
    case = rc.SCENES[name]()
    args, kw = rc.render_args(case)
    out = render.render_frames_numpy(_scene(case["meshes"], dtype), *args, **kw)
    assert not out["ambiguous"].any(), int(out["ambiguous"].sum())
    assert (out["px_vis"] > 0).sum() >= (7 if name == "two objects" else 1)
    if name == "two objects":
        occluded = (out["px_vis"][:, 0] < out["px_all"][:, 0])
        assert occluded[0] and occluded[2] and out["px_all"][1, 1] == 0   # object 1 hides a part of object 0 where it is drawn
