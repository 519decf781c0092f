#!/usr/bin/env python3
"""Generates tests/golden/pose_targets.npz from the REAL reference's ground-truth target computation.

Runs ONLY where the reference tree is mounted (the build container); nothing here travels to the GPU box except the .npz it writes.
At generation time it reads, and never stores:
  datasets/lm/linemod_pbr.py get_pose_gt_info (:602-655), the method text (method_text of make_golden.py), run with a stand-in
      `self` that has n_points and obj_mesh
  utils/compute_visibility.py VisiblePoints / sphericalFlip (scipy ConvexHull), with utils.ply stubbed
  utils/icp.py nearest_neighbor (sklearn NearestNeighbors), with cv2 stubbed
VisiblePoints is wrapped to record the camera centre the reference passes (inv_t.T, its float32 LAPACK inverse) and the flipped points.

Cases (model = synthetic.make_model_points, mm -> m; poses at 0.5-1.2 m):
  a  6 crops, one shared model, M=4096, N=2048, a few labelled points more than 1 cm off the model
  b  no labelled point (early return, :626-630)
  c  every labelled point more than 1 cm off (early return, :644-646)
  d  one model per crop (3 crops, M=1024)
  e  the camera inside the model's hull, so the origin is not a hull vertex and vertices[:-1] drops a model vertex
  f  one crop, N=4096, M=8192

Each case is regenerated (next seed) until it is stable:
  - the Qhull vertex set (with the origin) is unchanged when the flipped points are scaled by (1 + 1e-11 u), u uniform in [-1, 1]
    per coordinate, 3 draws, for both centres.  1e-11 relative is about 3e-8 m at the flipped radius (~3e3 m): four orders of
    magnitude above the fp64 rounding of either side (Qhull's arithmetic, the device's frame and constraint sums, ~1e-15 relative),
    so a vertex set that survives it does not depend on how the hull is computed;
  - no labelled point is within 1e-6 m of a nearest / second-nearest tie or of the 1 cm threshold (posed with both np.dot and the
    device's ((r0 x + r1 y) + r2 z) + t order): such a point is drawn again, so only the points are regenerated, not the case;
  - no model vertex and no flipped point is duplicated.
Stored per case: inputs, the reference inv_t, the visible sets for the reference centre and for the default centre
(targets.default_cam_center), the reference outputs, and the reference's flipped points of the small cases b and e (the CPU test
checks the documented flip formula against them, the GPU test the device's bits; the generator itself asserts that formula against
sphericalFlip for every crop).
"""
import math
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
os.environ.setdefault("MPLBACKEND", "Agg")

from geometric_aware_dense_matching_amd import synthetic  # noqa: E402
from geometric_aware_dense_matching_amd.targets import default_cam_center, spherical_flip  # noqa: E402

EPS_REL, TIE, THRESH = 1e-11, 1e-6, 0.01


def method_text(path, name, indent="    "):
    src = open(os.path.join(REF, path)).read().split("\n")
    a0 = next(i for i, l in enumerate(src) if l.startswith(indent + "def " + name + "("))
    a1 = next(i for i in range(a0 + 1, len(src)) if src[i].startswith(indent + "def ") or (src[i].strip() and not src[i].startswith(indent)))
    return textwrap.dedent("\n".join(src[a0:a1]))


def load_reference():
    assert os.path.isdir(REF), "reference tree not mounted"
    sys.path.insert(0, REF)

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("cv2")
    import utils  # noqa: F401  (namespace package of the reference)
    stub("utils.ply", load_ply=None)
    import utils.compute_visibility as CV
    import utils.icp as ICP
    rec = {}

    def visible_points(pts, cam_center):
        rec["inv_t"] = np.array(cam_center, dtype=np.float32).reshape(3)
        rec["flipped"] = CV.sphericalFlip(pts, cam_center, math.pi)
        rec["visible"] = CV.VisiblePoints(pts, cam_center)
        return rec["visible"]

    env = dict(np=np, VisiblePoints=visible_points, nearest_neighbor=ICP.nearest_neighbor)
    exec(method_text("datasets/lm/linemod_pbr.py", "get_pose_gt_info"), env)
    return env["get_pose_gt_info"], CV, rec


def rand_rot(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def hull_vertices(CV, f):
    return np.sort(CV.convexHull(f).vertices)


def stable_visibility(CV, model, c, rs):
    """The reference visible set for centre c, or None when a 1e-11 relative perturbation changes the hull's vertex set."""
    f = CV.sphericalFlip(model, c.reshape(1, 3), math.pi)
    if len(np.unique(f, axis=0)) != len(f):
        return None
    base = hull_vertices(CV, f)
    for _ in range(3):
        fp = f * (1.0 + EPS_REL * rs.uniform(-1, 1, size=f.shape))
        if not np.array_equal(hull_vertices(CV, fp), base):
            return None
    return CV.VisiblePoints(model, c.reshape(1, 3))


def pose_order(model, RT):
    R, t = RT[:, :3], RT[:, 3]
    x, y, z = model[:, 0], model[:, 1], model[:, 2]
    return np.stack([((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)], axis=1).astype(np.float32)


def make_model(seed, M, scale=1.0):
    return (synthetic.make_model_points(seed, M)[:, :3] * (scale / 1000.0)).astype(np.float32)


def make_pose(rs, inside=False):
    R = rand_rot(rs)
    if inside:
        t = (rs.uniform(-0.01, 0.01, size=3)).astype(np.float64)        # the camera within ~1 cm of the model centre
    else:
        t = np.array([rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1), rs.uniform(0.5, 1.2)])
    return np.concatenate([R, t[:, None]], axis=1).astype(np.float32)


def point_margins(pts, model, RT, vis):
    """Per point: False when it is within TIE of a nearest / second-nearest tie or of the threshold (posed both ways)."""
    ok = np.ones(len(pts), bool)
    for posed in (np.dot(model[vis], RT[:, :3].T) + RT[:, 3:].T, pose_order(model[vis], RT)):
        d = np.sqrt(((pts.astype(np.float64)[:, None, :] - posed.astype(np.float64)[None]) ** 2).sum(-1))
        d.sort(axis=1)
        ok &= (d[:, 1] - d[:, 0] >= TIE) & (np.abs(d[:, 0] - THRESH) >= TIE)
    return ok


def make_points(rs, model, RT, N, n_lab, far_frac, vis, all_far=False):
    """Labelled points on the camera-facing side of the posed model plus 1-2 mm noise (far_frac of them 1.5-3 cm off), the rest
    background; shuffled.  A labelled point that lands near a tie (point_margins) is drawn again.  -> cld f32[N,3], labels u8[N]."""
    posed = np.dot(model, RT[:, :3].T) + RT[:, 3:].T
    front = np.where(posed[:, 2] < np.median(posed[:, 2]))[0]
    far = rs.rand(n_lab) < far_frac if not all_far else np.ones(n_lab, bool)
    lab_pts = np.zeros((n_lab, 3), np.float32)
    todo = np.arange(n_lab)
    while len(todo):
        pick = rs.choice(front, size=len(todo))
        dirs = rs.randn(len(todo), 3)
        out = posed[pick] - posed.mean(0)                                   # far points move outwards, off the surface
        fo = far[todo]
        dirs[fo] = out[fo] / np.linalg.norm(out[fo], axis=1, keepdims=True) + 0.2 * dirs[fo]
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        off = rs.uniform(0.001, 0.002, size=(len(todo), 1))
        off[fo, 0] = rs.uniform(0.015, 0.03, size=fo.sum())
        lab_pts[todo] = (posed[pick] + dirs * off).astype(np.float32)
        todo = todo[~point_margins(lab_pts[todo], model, RT, vis)]
    bg = posed.mean(0) + rs.uniform(-0.15, 0.15, size=(N - n_lab, 3))
    cld = np.concatenate([lab_pts, bg]).astype(np.float32)
    labels = np.concatenate([np.ones(n_lab, np.uint8), np.zeros(N - n_lab, np.uint8)])
    order = rs.permutation(N)
    return cld[order], labels[order]


def mask_bits(idx, M):
    mk = np.zeros(M, np.uint8)
    mk[idx] = 1
    return np.packbits(mk)


def run_case(ref, CV, rec, rs, models, RTs, N, lab_counts, far_frac, all_far=False):
    """One case (B crops).  -> dict of arrays, or None when some crop is not stable."""
    B = len(RTs)
    out = {k: [] for k in ("cld", "labels", "inv_t", "vis_ref", "vis_def", "labels_out", "match_idx", "visible_flag", "valid")}
    flipped0 = None
    for b in range(B):
        model, RT = models[b], RTs[b]
        M = len(model)
        if len(np.unique(model, axis=0)) != M:
            return None
        T = np.eye(4, dtype=np.float32)                 # the reference's centre (linemod_pbr.py:617-623), checked below
        T[:3, :4] = RT
        inv_t = np.linalg.inv(T)[:3, 3].astype(np.float32)
        vis_ref = stable_visibility(CV, model, inv_t, rs)
        vis_def = stable_visibility(CV, model, default_cam_center(RT[None])[0], rs)
        if vis_ref is None or vis_def is None:
            return None
        cld, labels = make_points(rs, model, RT, N, lab_counts[b], far_frac, vis_ref, all_far)
        self = types.SimpleNamespace(n_points=M, obj_mesh=model)
        rec.clear()
        lab_o, match, vflag, valid = ref(self, cld, labels.copy(), {"pose": RT})
        if "inv_t" in rec:                              # no labelled point: the reference returns before its visibility
            assert np.array_equal(rec["inv_t"], inv_t) and np.array_equal(rec["visible"], vis_ref)
        f = CV.sphericalFlip(model, inv_t.reshape(1, 3), math.pi)
        assert np.array_equal(f, spherical_flip(model, inv_t)), "documented flip formula differs from sphericalFlip"
        if b == 0:
            flipped0 = f
        out["cld"].append(cld)
        out["labels"].append(labels)
        out["inv_t"].append(inv_t)
        out["vis_ref"].append(mask_bits(vis_ref, M))
        out["vis_def"].append(mask_bits(vis_def, M))
        out["labels_out"].append(lab_o.astype(np.uint8))
        out["match_idx"].append(match.astype(np.int16 if M < 32767 else np.int32))
        out["visible_flag"].append(np.packbits(vflag.astype(np.uint8)))
        out["valid"].append(bool(valid))
    res = {k: np.stack(v) for k, v in out.items()}
    res["RT"] = np.stack(RTs)
    res["flipped0"] = flipped0
    return res


def main():
    ref, CV, rec = load_reference()
    specs = {
        # name: (B, M, N, labelled per crop, far fraction, shared model, inside, all_far, store flipped0)
        "a": (6, 4096, 2048, 1000, 0.01, True, False, False, False),
        "b": (1, 1024, 512, 0, 0.0, True, False, False, True),
        "c": (1, 1024, 512, 200, 1.0, True, False, True, False),
        "d": (3, 1024, 512, 250, 0.05, False, False, False, False),
        "e": (1, 1024, 512, 200, 0.05, True, True, False, True),
        "f": (1, 8192, 4096, 2000, 0.01, True, False, False, False),
    }
    arrays = {}
    for name, (B, M, N, n_lab, far, shared, inside, all_far, keep_f) in specs.items():
        for seed in range(1, 200):
            rs = np.random.RandomState(1000 * (ord(name) - 96) + seed)
            if shared:
                m = make_model(seed, M)
                models = [m] * B
            else:
                models = [make_model(seed * 10 + b, M, scale=rs.uniform(0.8, 1.2)) for b in range(B)]
            RTs = [make_pose(rs, inside) for _ in range(B)]
            res = run_case(ref, CV, rec, rs, models, RTs, N, [n_lab] * B, far, all_far)
            if res is None:
                print("case %s seed %d: unstable, next" % (name, seed))
                continue
            res["model"] = models[0] if shared else np.stack(models)
            if not keep_f:
                res.pop("flipped0")
            for k, v in res.items():
                arrays["%s_%s" % (name, k)] = v
            print("case %s seed %d: B=%d M=%d N=%d valid=%s visible(ref)=%s" % (
                name, seed, B, M, N, res["valid"].tolist(), [int(np.unpackbits(v)[:M].sum()) for v in res["vis_ref"]]))
            break
        else:
            raise SystemExit("case %s: no stable seed" % name)
    path = os.path.join(HERE, "pose_targets.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
