"""Per-instance pose errors for a whole batch on the GPU and the reference's recall tables.

Mirrors /root/reference/evaluator.py:308-463 (`Evaluator._eval_predictions`) with its error functions
  lib/pysixd/pose_error.py:297-337 add / adi, :400-415 re, :425-437 te, :440-445 arp_2d, utils/pose_utils.py:430-454 get_closest_rot
but batched: the reference walks the predictions one instance at a time in numpy; here a batch of estimated and ground-truth poses of
ONE object goes through a handful of tensor operations on the device (ADI's nearest neighbour is the HIP kNN kernel, pose.py), and only the
per-instance scalars come back to the host for the table.  Units as in the reference: metres, degrees, pixels; diameters in metres.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import pixel_rule, pose

METRICS = ["ad_2", "ad_5", "ad_10", "ad_0.1", "rete_2", "rete_5", "rete_10", "re_2", "re_5", "re_10", "te_2", "te_5", "te_10",
           "proj_2", "proj_5", "proj_10"]                           # evaluator.py:323-340


def rotation_error_deg(R_est, R_gt):
    """pose_error.py:400-415 for f[n,3,3] batches -> degrees f[n] (computed in fp64: the arccos near 0 needs it)."""
    tr = torch.einsum("nij,nij->n", R_est.double(), R_gt.double())          # trace(R_est R_gt^T)
    cos = (0.5 * (tr.clamp(max=3.0) - 1.0)).clamp(-1.0, 1.0)
    return torch.rad2deg(torch.arccos(cos))


def closest_symmetric_rotation(R_est, R_gt, sym_rots):
    """pose_utils.py:430-454 for batches: among R_gt and R_gt @ S_k the rotation with the smallest error to R_est (the first wins ties,
    R_gt itself before any symmetric copy, as the reference's strict `<` does).  sym_rots f[K,3,3] (model-to-model) or None."""
    if sym_rots is None or len(sym_rots) == 0:
        return R_gt
    S = torch.as_tensor(sym_rots, dtype=R_gt.dtype, device=R_gt.device).reshape(-1, 3, 3)
    cands = torch.cat([R_gt[:, None], torch.einsum("nij,kjl->nkil", R_gt, S)], dim=1)       # [n, 1+K, 3, 3]
    n, k = cands.shape[:2]
    errs = rotation_error_deg(R_est[:, None].expand(n, k, 3, 3).reshape(-1, 3, 3), cands.reshape(-1, 3, 3)).view(n, k)
    best = torch.argmin(errs, dim=1)                                # argmin returns the first minimum
    return cands[torch.arange(n, device=R_gt.device), best]


def reprojection_error_px(RT_est, RT_gt, model_xyz, K):
    """pose_error.py:440-445 (arp_2d): mean pixel distance of the model vertices projected with both poses.  K f[3,3] or f[n,3,3]."""
    Kt = torch.as_tensor(K, dtype=torch.float64, device=RT_est.device)
    Kt = Kt.expand(RT_est.shape[0], 3, 3) if Kt.dim() == 2 else Kt

    def project(RT):
        pc = torch.einsum("nij,nmj->nmi", Kt, pose.transform(model_xyz.double(), RT.double()))
        return pc[..., :2] / pc[..., 2:3]
    return (project(RT_est) - project(RT_gt)).norm(dim=2).mean(dim=1)


def pose_errors(RT_est, RT_gt, model_xyz, K, symmetric=False, sym_rots=None):
    """evaluator.py:378-400 for n instances of one object: RT f32[n,3,4] (model -> camera), model_xyz f32[M,3] (metres) ->
    dict(ad, re, te, proj) of f64[n] on the device.  Symmetric objects: ADI, and re / proj against the closest symmetric ground truth."""
    RT_est = RT_est.float()
    RT_gt = RT_gt.to(RT_est.device).float()
    te = (RT_gt[:, :, 3].double() - RT_est[:, :, 3].double()).norm(dim=1)
    if symmetric:
        R_sym = closest_symmetric_rotation(RT_est[:, :, :3], RT_gt[:, :, :3], sym_rots)
        RT_sym = torch.cat([R_sym, RT_gt[:, :, 3:]], dim=2)
        re = rotation_error_deg(RT_est[:, :, :3], R_sym)
        proj = reprojection_error_px(RT_est, RT_sym, model_xyz, K)
        ad = pose.adi_metric(RT_est, RT_gt, model_xyz).double()
    else:
        re = rotation_error_deg(RT_est[:, :, :3], RT_gt[:, :, :3])
        proj = reprojection_error_px(RT_est, RT_gt, model_xyz, K)
        ad = pose.add_metric(RT_est, RT_gt, model_xyz).double()
    return dict(ad=ad, re=re, te=te, proj=proj)


PRECISION_METRICS = [m for m in METRICS if m != "ad_0.1"]          # evaluator.py:513-529: the precision table has no absolute 10 cm line


class RecallTable:
    """The recall / error bookkeeping of evaluator.py:342-463.  update() takes the errors of a batch of instances of one object,
    missing() records ground truths without a prediction (every recall 0, no error entry: :359-362), table() / format() give the
    reference's table: one line per metric with the per-object mean recall x 100 and the mean over objects, then mean re / te.

    precision=True is `_eval_predictions_precision` (evaluator.py:466-660, "precision as in the DPOD paper"): ground truths without a
    prediction are IGNORED instead of counted as misses (:549-551) and the metric list drops "ad_0.1"; everything else is the same
    bookkeeping.  dump() writes what the reference leaves in its output directory (:449-455 / :647-660)."""

    def __init__(self, precision=False):
        self.precision = bool(precision)
        self.metrics = PRECISION_METRICS if self.precision else METRICS
        self.recalls = OrderedDict()
        self.errors = OrderedDict()

    def _slot(self, obj_name):
        if obj_name not in self.recalls:
            self.recalls[obj_name] = OrderedDict((m, []) for m in self.metrics)
            self.errors[obj_name] = OrderedDict((e, []) for e in ("ad", "re", "te", "proj"))
        return self.recalls[obj_name], self.errors[obj_name]

    def missing(self, obj_name, count=1):
        rec, _ = self._slot(obj_name)
        if self.precision:
            return                                                      # "NOTE: just ignore undetected" (evaluator.py:549-551)
        for m in self.metrics:
            rec[m] += [0.0] * count

    def dump(self, output_dir, dataset_name, method_name=""):
        """errors / recalls as pickles and the table as text, under the reference's file names: `_{dataset}_errors.pkl`,
        `_{dataset}_recalls.pkl`, `_{dataset}_tab.txt` (evaluator.py:449-455); the precision variant prefixes the method name and
        says `precisions` (:647-660).  The reference writes the pickles through mmcv.dump, which is pickle for a .pkl path."""
        import os
        import pickle
        os.makedirs(output_dir, exist_ok=True)
        kind = "precisions" if self.precision else "recalls"
        stem = os.path.join(output_dir, "%s_%s" % (method_name, dataset_name))
        paths = (stem + "_errors.pkl", stem + "_%s.pkl" % kind, stem + ("_tab_precisions.txt" if self.precision else "_tab.txt"))
        with open(paths[0], "wb") as f:
            pickle.dump(self.errors, f)
        with open(paths[1], "wb") as f:
            pickle.dump(self.recalls, f)
        with open(paths[2], "w") as f:
            f.write("%s\n" % self.format())
        return paths


    def update(self, obj_name, errors, diameter):
        """errors: pose_errors() output (tensors or arrays of equal length); diameter in metres."""
        rec, err = self._slot(obj_name)
        e = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float64) for k, v in errors.items()}
        for k in err:
            err[k] += e[k].tolist()
        ad, re, te, proj = e["ad"], e["re"], e["te"], e["proj"]
        flags = {"ad_2": ad < 0.02 * diameter, "ad_5": ad < 0.05 * diameter, "ad_10": ad < 0.1 * diameter, "ad_0.1": ad < 0.1,
                 "rete_2": (re < 2) & (te < 0.02), "rete_5": (re < 5) & (te < 0.05), "rete_10": (re < 10) & (te < 0.1),
                 "re_2": re < 2, "re_5": re < 5, "re_10": re < 10, "te_2": te < 0.02, "te_5": te < 0.05, "te_10": te < 0.1,
                 "proj_2": proj < 2, "proj_5": proj < 5, "proj_10": proj < 10}           # evaluator.py:408-427
        for m in self.metrics:
            rec[m] += flags[m].astype(np.float64).tolist()

    def table(self):
        obj_names = sorted(self.recalls.keys())
        tab = [["objects"] + obj_names + ["Avg(%d)" % len(obj_names)]]
        for m in self.metrics:
            line, vals = [m], []
            for o in obj_names:
                res = self.recalls[o][m]
                line.append("%.2f" % (100 * np.mean(res)) if len(res) > 0 else 0.0)
                vals.append(np.mean(res) if len(res) > 0 else 0.0)
            if obj_names:
                line.append("%.2f" % (100 * np.mean(vals)))
            tab.append(line)
        for e in ("re", "te"):
            line, vals = [e], []
            for o in obj_names:
                res = self.errors[o][e]
                line.append("%.2f" % np.mean(res) if len(res) > 0 else float("nan"))
                vals.append(np.mean(res) if len(res) > 0 else float("nan"))
            if obj_names:
                line.append("%.2f" % np.mean(vals))
            tab.append(line)
        return tab

    def format(self):
        tab = [[str(c) for c in row] for row in self.table()]
        width = [max(len(r[i]) for r in tab if i < len(r)) for i in range(max(len(r) for r in tab))]
        return "\n".join("  ".join(c.ljust(width[i]) for i, c in enumerate(r)).rstrip() for r in tab)


class BopCsv:
    """The BOP-toolkit result file the reference writes while it walks the predictions (evaluator.py:341,365-373,429-431): header
    `scene_id,im_id,obj_id,score,R,t,time`, one line per predicted instance with R row-major and t in MILLIMETRES, both space
    separated, time -1 and score -1 unless one is given.  `file_name` is the reference's prediction key "scene/…/im_id" (:366-367)."""

    HEADER = "scene_id,im_id,obj_id,score,R,t,time"

    def __init__(self):
        self.lines = [self.HEADER]

    def add(self, file_name, obj_id, R, t, score=-1, time=-1):
        R = np.asarray(R.detach().cpu() if torch.is_tensor(R) else R, dtype=np.float64).reshape(3, 3)
        t = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float64).reshape(-1)
        parts = str(file_name).split("/")
        self.lines.append("{scene_id},{im_id},{obj_id},{score},{R},{t},{time}".format(
            scene_id=int(parts[0]), im_id=parts[-1], obj_id=int(obj_id), score=score,
            R=" ".join(map(str, R.flatten().tolist())), t=" ".join(map(str, (t * 1000).flatten().tolist())), time=time))

    def add_batch(self, file_names, obj_id, RT, scores=None):
        """RT [n,3,4] (pose.solve_poses / infer.run_multi_object output), metres; scores [n] (the step's `score` with soft matching)
        are written when given, -1 otherwise."""
        RT = RT.detach().cpu().double().numpy() if torch.is_tensor(RT) else np.asarray(RT, dtype=np.float64)
        if scores is None:
            for name, rt in zip(file_names, RT):
                self.add(name, obj_id, rt[:, :3], rt[:, 3])
            return
        scores = scores.detach().cpu().double().numpy() if torch.is_tensor(scores) else np.asarray(scores, dtype=np.float64)
        if scores.shape != (len(RT),):
            raise ValueError("BopCsv.add_batch: %d poses, scores of shape %s" % (len(RT), scores.shape))
        for name, rt, sc in zip(file_names, RT, scores):
            self.add(name, obj_id, rt[:, :3], rt[:, 3], score=float(sc))

    def write(self, path):
        import os
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(self.lines))                             # no trailing newline, as the reference (:430-431)
        return path


# ------------------------------------------------------------------------------------------------------------------------------------
# BOP pose errors: MSSD, MSPD, VSD (lib/pysixd/pose_error.py:22-179) with the symmetry sets of lib/pysixd/misc.py:206-254 and the
# visibility masks of lib/pysixd/visibility.py.  The device paths are gdm_bop.hip (ops.mssd_mspd / render_depth / vsd_counts); the
# *_numpy functions restate them in fp64 on the host, operation for operation where a result is decided.

BOP_THETAS = np.round(np.arange(1, 11) * 0.05, 2)                   # BOP-2019: correct when e < theta (x diameter for MSSD, VSD as is)
BOP_MSPD_THETAS = np.arange(1, 11) * 5.0                            # pixels at a 640 px wide image
BOP_VSD_TAUS = np.round(np.arange(1, 11) * 0.05, 2)                 # misalignment tolerances, fractions of the diameter
BOP_VSD_DELTA = 0.015                                               # 15 mm, in metres: multiply by the caller's units per metre


def load_models_info(path):
    """models_info.json of a BOP dataset -> {obj_id (int): info dict}."""
    import json
    with open(path) as f:
        return {int(k): v for k, v in json.load(f).items()}


def _axis_rotation(angle, axis):
    """lib/pysixd/transform.py:295-335 (rotation_matrix) without the point: 3x3."""
    sina, cosa = np.sin(angle), np.cos(angle)
    d = np.asarray(axis, dtype=np.float64)[:3]
    d = d / np.sqrt(np.dot(d, d))
    R = np.diag([cosa, cosa, cosa]) + np.outer(d, d) * (1.0 - cosa)
    d = d * sina
    return R + np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])


def symmetry_transformations(model_info, max_sym_disc_step=0.01, scale=1.0):
    """misc.get_symmetry_transformations (misc.py:206-254) -> R f64[S,3,3], t f64[S,3].  The discrete list is the identity first, then the
    flat 4x4 lists of `symmetries_discrete`; every continuous symmetry is discretised into ceil(pi / step) steps about `axis` through
    `offset` (the zero rotation left out); with continuous symmetries the set is, for each discrete one, all continuous ones composed
    in front of it -- the reference's order, which then holds no identity.  t stays in the model
    file's unit (mm in BOP) times `scale` (0.001 for this project's metres)."""
    disc = [(np.eye(3), np.zeros(3))]
    for sym in model_info.get("symmetries_discrete", ()):
        m = np.reshape(np.asarray(sym, dtype=np.float64), (4, 4))
        disc.append((m[:3, :3], m[:3, 3]))
    cont = []
    for sym in model_info.get("symmetries_continuous", ()):
        offset = np.asarray(sym["offset"], dtype=np.float64).reshape(3)
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(1, steps):
            R = _axis_rotation(i * step, sym["axis"])
            cont.append((R, -R.dot(offset) + offset))
    out = []
    for Rd, td in disc:
        if cont:
            out += [(Rc.dot(Rd), Rc.dot(td) + tc) for Rc, tc in cont]
        else:
            out.append((Rd, td))
    return np.stack([r for r, _ in out]).astype(np.float64), np.stack([t for _, t in out]).astype(np.float64) * float(scale)


def _np64(x):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float64)


def mssd_mspd_numpy(RT_est, RT_gt, pts, sym_R, sym_t, K):
    """pose_error.py:131-179 in fp64 numpy, one instance and one symmetry at a time as the reference walks them: the same outputs as
    mssd_mspd (numpy arrays).  The first minimum wins a tie (the reference's min())."""
    RT_est, RT_gt, pts, sym_R, sym_t, K = (_np64(a) for a in (RT_est, RT_gt, pts, sym_R, sym_t, K))
    n = RT_est.shape[0]
    K = np.broadcast_to(K, (n, 3, 3))
    pts_h = np.hstack([pts, np.ones((pts.shape[0], 1))])

    def project(Kb, R, t):                                          # misc.project_pts (misc.py:511-525)
        im = Kb.dot(np.hstack([R, t.reshape(3, 1)])).dot(pts_h.T)
        return (im[:2] / im[2]).T

    mssd, mspd = np.zeros(n), np.zeros(n)
    b3, b2 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        Re, te, Rg, tg = RT_est[i, :, :3], RT_est[i, :, 3], RT_gt[i, :, :3], RT_gt[i, :, 3]
        pe, ue = pts.dot(Re.T) + te, project(K[i], Re, te)
        e3, e2 = [], []
        for Rs, ts in zip(sym_R, sym_t):
            Rgs, tgs = Rg.dot(Rs), Rg.dot(ts) + tg
            e3.append(np.linalg.norm(pe - (pts.dot(Rgs.T) + tgs), axis=1).max())
            e2.append(np.linalg.norm(ue - project(K[i], Rgs, tgs), axis=1).max())
        b3[i], b2[i] = int(np.argmin(e3)), int(np.argmin(e2))
        mssd[i], mspd[i] = e3[b3[i]], e2[b2[i]]
    return mssd, mspd, b3, b2


def _f64dev(x, device):
    return torch.as_tensor(x).to(device=device, dtype=torch.float64)


def mssd_mspd(RT_est, RT_gt, pts, sym_R, sym_t, K):
    """MSSD and MSPD (pose_error.py:131-179) of n pose pairs of ONE object in one kernel: RT_est (a device tensor) and RT_gt [n,3,4],
    pts [M,3], sym_R [S,3,3] / sym_t [S,3] (symmetry_transformations; t in the unit of pts), K [3,3] or [n,3,3] -> mssd f64[n] (unit
    of pts), mspd f64[n] (pixels), best_sym_mssd i32[n], best_sym_mspd i32[n] on the device.  Inputs of any float dtype are widened to
    fp64 there; no [n,S,M] array exists at any point (the largest temporary is [2,n,S])."""
    from . import ops
    dev = RT_est.device
    return ops.mssd_mspd(_f64dev(RT_est, dev), _f64dev(RT_gt, dev)[:, :3], _f64dev(pts, dev), _f64dev(sym_R, dev), _f64dev(sym_t, dev),
                         _f64dev(K, dev))


def render_depth_numpy(verts, faces, RT, K, H, W, near):
    """The pixel rule of include/gdm.h (gdm_render_depth_hip) on the host, the definition the kernel is tested against:
    fp64 vertex transform ((R_i0 x + R_i1 y) + R_i2 z) + t_i, u = fx (X / Z) + cx (skew ignored, pixel centres at integers), snapping
    to 1/256 px, int64 edge functions with the top-left rule on the winding normalised by the sign of the area, perspective-correct
    depth, minimum over the triangles in the unsigned order of the depth bits -> f32[n,H,W], 0 where nothing is drawn.  The rule
    itself is pixel_rule.project and pixel_rule.covered; this function keeps the z-buffer."""
    verts, RT, K = _np64(verts), _np64(RT), _np64(K)
    faces = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64)
    n = RT.shape[0]
    K = np.broadcast_to(K, (n, 3, 3))
    out = np.full((n, H, W), pixel_rule.INF_BITS, dtype=np.uint32)
    for b in range(n):
        for _, (px0, py0, px1, py1), inside, d in pixel_rule.covered(faces, *pixel_rule.project(verts, RT[b], K[b], near), H, W):
            tile = out[b, py0:py1 + 1, px0:px1 + 1]
            tile[inside] = np.minimum(tile[inside], pixel_rule.depth_keys(d)[inside])
    out[out >= pixel_rule.INF_BITS] = 0
    return out.view(np.float32)


def render_depth(verts, faces, RT, K, H, W, near, keep_inf=False):
    """Depth images of a triangle mesh in n poses on the device (ops.render_depth): verts f32|f64[V,3] and faces i32[F,3] (device
    tensors or arrays), RT [n,3,4] a device tensor, K [3,3] or [n,3,3] -> f32[n,H,W], 0 where nothing is drawn.  The image is defined
    by the written pixel rule (render_depth_numpy restates it; only fx, fy, cx, cy of K are used: skew is ignored) and is reproducible
    bit for bit.  Parity with BOP's OpenGL renderers is NOT pinned."""
    from . import ops
    dev = RT.device
    verts = torch.as_tensor(verts).to(dev)
    if verts.dtype not in (torch.float32, torch.float64):
        verts = verts.double()
    return ops.render_depth(verts, torch.as_tensor(faces).to(device=dev, dtype=torch.int32), _f64dev(RT, dev)[:, :3], _f64dev(K, dev),
                            H, W, near, keep_inf=keep_inf)


def _vsd_masks_numpy(depth_est, depth_gt, depth_test, K, delta):
    """One instance: the fp64 distance images (misc.py:571-590) and the bop19 visibility masks (visibility.py:34-36, 72-73)."""
    H, W = depth_test.shape
    pre_x = (np.arange(W, dtype=np.float64)[None, :] - K[0, 2]) / np.float64(K[0, 0])
    pre_y = (np.arange(H, dtype=np.float64)[:, None] - K[1, 2]) / np.float64(K[1, 1])

    def dist(d):
        return np.sqrt(np.multiply(pre_x, d) ** 2 + np.multiply(pre_y, d) ** 2 + d.astype(np.float64) ** 2)

    dist_t, dist_g, dist_e = dist(depth_test), dist(depth_gt), dist(depth_est)
    t32, no_test = dist_t.astype(np.float32), dist_t == 0

    def visible(d_model):
        return ((d_model.astype(np.float32) - t32 <= np.float32(delta)) | no_test) & (d_model > 0)

    vis_g = visible(dist_g)
    vis_e = visible(dist_e) | (vis_g & (dist_e > 0))
    return dist_t, dist_g, dist_e, vis_g, vis_e


def vsd_numpy(depth_est, depth_gt, depth_test, K, delta, taus, diameter=None, cost_type="step", return_counts=False):
    """pose_error.py:84-126 on given depth images in fp64 numpy, the arithmetic of gdm_vsd_counts_hip operation for operation:
    depth_est / depth_gt f32[n,H,W], depth_test f32[H,W] or [n,H,W], K [3,3] or [n,3,3] -> errors f64[n,T]; with return_counts also
    union i64[n], inter i64[n], cost i64[n,T] (cost_type "step")."""
    as32 = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float32)  # noqa: E731
    depth_est, depth_gt, depth_test, K = as32(depth_est), as32(depth_gt), as32(depth_test), _np64(K)
    n = depth_est.shape[0]
    K = np.broadcast_to(K, (n, 3, 3))
    taus = [float(t) for t in taus]
    errors = np.ones((n, len(taus)))
    union, inter, cost = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, len(taus)), np.int64)
    for b in range(n):
        _, dist_g, dist_e, vis_g, vis_e = _vsd_masks_numpy(depth_est[b], depth_gt[b], depth_test if depth_test.ndim == 2 else depth_test[b],
                                                           K[b], delta)
        both = vis_g & vis_e
        union[b], inter[b] = (vis_g | vis_e).sum(), both.sum()
        dists = np.abs(dist_g[both] - dist_e[both])
        if diameter:
            dists = dists / float(diameter)
        for j, tau in enumerate(taus):
            if cost_type == "step":
                cost[b, j] = c = (dists >= tau).sum()
            elif cost_type == "tlinear":
                c = np.minimum(dists / tau, 1.0).sum()
            else:
                raise ValueError("Unknown pixel matching cost.")
            if union[b] > 0:
                errors[b, j] = (c + (union[b] - inter[b])) / float(union[b])
    return (errors, union, inter, cost) if return_counts else errors


def _vsd_errors(counts, cost_type):
    if cost_type == "step":
        union, inter, cost = counts
        c = cost.double()
    elif cost_type == "tlinear":
        union, inter, _, c = counts
    else:
        raise ValueError("Unknown pixel matching cost.")
    u = union.double()[:, None]
    e = (c + (union - inter).double()[:, None]) / u
    return torch.where(u > 0, e, torch.ones_like(e))                # an empty union: 1.0 (pose_error.py:110-111)


def vsd(depth_est, depth_gt, depth_test, K, delta, taus, diameter=None, cost_type="step"):
    """The visible surface discrepancy (pose_error.py:84-126, visib_mode bop19) of n instances on given depth images, one kernel:
    depth_est / depth_gt f32[n,H,W] device tensors, depth_test f32[H,W] (shared) or [n,H,W], K [3,3] or [n,3,3]; delta and the pixel
    distances in the depth images' unit; the distances are divided by `diameter` when one is given (taus are then fractions of it)
    -> errors f64[n,T] on the device.  cost_type "step" is exact integer counting; "tlinear" sums in fp64."""
    from . import ops
    dev = depth_est.device
    counts = ops.vsd_counts(depth_est, depth_gt.to(dev), torch.as_tensor(depth_test).to(dev), _f64dev(K, dev), delta, taus, diameter,
                            tlinear=cost_type == "tlinear")
    return _vsd_errors(counts, cost_type)


def vsd_from_poses(verts, faces, RT_est, RT_gt, depth_test, K, delta, taus, diameter=None, cost_type="step", near=0.0,
                   return_counts=False):
    """VSD from poses: both poses of every instance are rendered in ONE rasteriser call (render_depth's pixel rule) and scored by
    the VSD kernel, which also reads the cleared z-buffer as empty; no depth image visits the host.  verts / faces: the object's mesh
    (load_ply); RT_est, RT_gt [n,3,4]; depth_test f32[H,W] or [n,H,W] on the device; K [3,3] or [n,3,3] -> errors f64[n,T] (with
    return_counts also the ops-level counts)."""
    from . import ops
    dev = RT_est.device
    depth_test = torch.as_tensor(depth_test).to(dev)
    H, W = depth_test.shape[-2:]
    n = RT_est.shape[0]
    K = _f64dev(K, dev)
    RT = torch.cat([_f64dev(RT_est, dev)[:, :3], _f64dev(RT_gt, dev)[:, :3]], dim=0)
    d = render_depth(verts, faces, RT, torch.cat([K, K], dim=0) if K.dim() == 3 else K, H, W, near, keep_inf=True)
    counts = ops.vsd_counts(d[:n], d[n:], depth_test, K, delta, taus, diameter, tlinear=cost_type == "tlinear", inf_is_empty=True)
    errors = _vsd_errors(counts, cost_type)
    return (errors, counts) if return_counts else errors


def _ply_faces(f, path, fmt, count, props, np_type, texcoords):
    """The `face` element: (faces i32[count,3], face texcoords f32[count,3,2] or None).  One list property of vertex indices; beside
    it scalar properties (skipped) and a list property `texcoord` (MeshLab's six floats per face; read only with `texcoords`, and then
    accepted only when every face has 3 indices and 6 coordinates)."""
    lists = [p for p in props if p[0] == "list"]
    index = [p for p in lists if p[3] in ("vertex_indices", "vertex_index")] or lists[:1]
    other = [p for p in lists if p is not index[0] and p[3] != "texcoord"]
    if len(index) != 1 or other:
        raise ValueError("%s: element 'face' with list properties %s is not supported" % (path, [p[3] for p in lists]))
    want = {id(index[0]): 3}
    want.update({id(p): 6 for p in lists if p[3] == "texcoord"})
    got = {}
    if fmt == "ascii" and len(props) == 1:
        rows = np.array([f.readline().split() for _ in range(count)], dtype=np.int64).reshape(count, -1)
        if rows.shape[1] != 4:
            raise ValueError("%s: faces must be triangles" % path)
        got[id(index[0])] = (rows[:, 0], rows[:, 1:4])
    elif fmt == "ascii":
        cols = {id(p): ([], []) for p in lists}
        for _ in range(count):
            tok, at = f.readline().split(), 0
            for p in props:
                if p[0] != "list":
                    at += 1
                    continue
                k = int(tok[at])
                cols[id(p)][0].append(k)
                cols[id(p)][1].append(tok[at + 1:at + 1 + k])
                at += 1 + k
        for p in lists:
            cnt = np.asarray(cols[id(p)][0], dtype=np.int64)
            ok = bool((cnt == want[id(p)]).all())
            got[id(p)] = (cnt, np.asarray(cols[id(p)][1], dtype=np.float64).reshape(count, want[id(p)]) if ok else None)
    else:                                                                  # binary: a fixed record, which the counts then confirm
        fields = []
        for k, p in enumerate(props):
            if p[0] == "list":
                fields += [("n%d" % k, "<" + np_type[p[1]]), ("v%d" % k, "<" + np_type[p[2]], (want[id(p)],))]
            else:
                fields.append(("s%d" % k, "<" + np_type[p[0]]))
        dt = np.dtype(fields)
        rec = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        for k, p in enumerate(props):
            if p[0] == "list":
                got[id(p)] = (rec["n%d" % k], rec["v%d" % k])
    cnt, idx = got[id(index[0])]
    if count and not (np.asarray(cnt) == 3).all():
        raise ValueError("%s: faces must be triangles" % path)
    faces = np.ascontiguousarray(idx).astype(np.int32).reshape(count, 3)
    fuv = None
    for p in lists:
        if p[3] == "texcoord" and (texcoords or fmt != "ascii"):           # a binary record was read on the strength of these counts
            cnt, val = got[id(p)]
            if count and not (np.asarray(cnt) == 6).all():
                raise ValueError("%s: the face property `texcoord` must hold 6 coordinates for every face (3 corners), found counts %s"
                                 % (path, sorted(set(int(c) for c in np.asarray(cnt)))[:4]))
            fuv = np.ascontiguousarray(val).astype(np.float32).reshape(count, 3, 2)
    return faces, fuv


def load_ply(path, attributes=False, texcoords=False):
    """The triangle meshes BOP ships, in pure numpy: ascii or binary_little_endian PLY with a `vertex` element whose properties include
    x, y, z and a `face` element with one list property of uchar / int (or uint) triples -> verts f64[V,3] (the file's unit: mm in
    BOP), faces i32[F,3].  attributes=True: also normals f32[V,3] from nx, ny, nz and colors u8[V,3] from red, green, blue, each None
    when the file lacks one of its three properties.  texcoords=True: also, at the end of the tuple, uv f32[F,3,2] -- one (u, v) per
    face corner, from the vertex properties texture_u / texture_v (BOP's form; also u / v or s / t) gathered through the faces, or from
    a face list property `texcoord` of six floats (MeshLab's form, which can hold a seam without doubled vertices) -- or None, and
    texture_file, the name after `comment TextureFile`, or None.  The image itself is not read here (texture.load_texture)."""
    np_type = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8",
               "int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "float32": "f4", "float64": "f8"}
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s is not a PLY file" % path)
        fmt, elements, texture_file = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header without end_header" % path)
            tok = line.decode("ascii", "replace").split()
            if len(tok) >= 3 and tok[0] == "comment" and tok[1] == "TextureFile" and texture_file is None:
                texture_file = " ".join(tok[2:])
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                elements[-1][2].append(tuple(tok[1:]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError("%s: PLY format %r is not supported (ascii, binary_little_endian)" % (path, fmt))
        verts = faces = normals = colors = vuv = fuv = None
        for name, count, props in elements:
            is_list = [p[0] == "list" for p in props]
            if any(is_list) and name != "face":
                raise ValueError("%s: element %r with list properties is not supported" % (path, name))
            if name == "face":
                faces, fuv = _ply_faces(f, path, fmt, count, props, np_type, texcoords)
            else:
                names = [p[1] for p in props]
                if fmt == "ascii":
                    rows = np.array([f.readline().split() for _ in range(count)], dtype=np.float64).reshape(count, len(props))
                    cols = {nm: rows[:, i] for i, nm in enumerate(names)}
                else:
                    dt = np.dtype([(nm, "<" + np_type[p[0]]) for nm, p in zip(names, props)])
                    rec = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
                    cols = {nm: rec[nm] for nm in names}
                if name == "vertex":
                    verts = np.stack([cols["x"], cols["y"], cols["z"]], axis=1).astype(np.float64)
                    if attributes and all(k in cols for k in ("nx", "ny", "nz")):
                        normals = np.stack([cols["nx"], cols["ny"], cols["nz"]], axis=1).astype(np.float32)
                    if attributes and all(k in cols for k in ("red", "green", "blue")):
                        colors = np.stack([cols["red"], cols["green"], cols["blue"]], axis=1).astype(np.uint8)
                    for ku, kv in (("texture_u", "texture_v"), ("u", "v"), ("s", "t")):
                        if texcoords and vuv is None and ku in cols and kv in cols:
                            vuv = np.stack([cols[ku], cols[kv]], axis=1).astype(np.float32)
    if verts is None or faces is None:
        raise ValueError("%s: PLY without a vertex and a face element" % path)
    out = (verts, faces, normals, colors) if attributes else (verts, faces)
    if not texcoords:
        return out
    if fuv is None and vuv is not None:
        if len(faces) and (faces.min() < 0 or faces.max() >= len(vuv)):
            raise ValueError("%s: a face index lies outside [0, %d)" % (path, len(vuv)))
        fuv = np.ascontiguousarray(vuv[faces.astype(np.int64)])
    return out + (fuv, texture_file)


class BopScores:
    """The BOP-2019 scores beside RecallTable: for every object the recall of MSSD (correct when e < theta x diameter, theta = 0.05
    ... 0.5), MSPD (e < theta x width / 640 px, theta = 5 ... 50) and VSD (e < theta for the same ten theta as MSSD, over the ten
    misalignment tolerances tau = 0.05 ... 0.5 of the diameter the errors were computed at, BOP_VSD_TAUS, with delta = BOP_VSD_DELTA),
    AR_x = the mean recall over the thresholds of error x and AR = the mean of the three (of the two when no VSD was given).

    update() takes the errors of a batch of instances of one object, missing() records ground truths without an estimate (every
    recall 0).  There is ONE estimate per ground-truth instance, as everywhere in this evaluator: the toolkit's matching of several
    estimates to the instances of an image (eval_calc_scores.py) is not restated."""

    def __init__(self):
        self.correct = OrderedDict()                                # obj -> {"mssd": [bool[10]], "mspd": [bool[10]], "vsd": [bool[10, T]]}
        self.errors = OrderedDict()

    def _slot(self, obj_name):
        if obj_name not in self.correct:
            self.correct[obj_name] = OrderedDict((e, []) for e in ("mssd", "mspd", "vsd"))
            self.errors[obj_name] = OrderedDict((e, []) for e in ("mssd", "mspd", "vsd"))
        return self.correct[obj_name], self.errors[obj_name]

    def update(self, obj_name, mssd, mspd, vsd=None, diameter=1.0, width=640):
        """mssd f[n] (unit of `diameter`), mspd f[n] (pixels), vsd f[n,T] or None (errors at the T tolerances), tensors or arrays."""
        cor, err = self._slot(obj_name)
        mssd, mspd = _np64(mssd).reshape(-1), _np64(mspd).reshape(-1)
        err["mssd"] += mssd.tolist()
        err["mspd"] += mspd.tolist()
        cor["mssd"] += list(mssd[:, None] < BOP_THETAS[None, :] * float(diameter))
        cor["mspd"] += list(mspd[:, None] < BOP_MSPD_THETAS[None, :] * (float(width) / 640.0))
        if vsd is not None:
            vsd = _np64(vsd).reshape(len(mssd), -1)
            err["vsd"] += vsd.tolist()
            cor["vsd"] += list(vsd[:, None, :] < BOP_THETAS[None, :, None])

    def missing(self, obj_name, count=1, vsd_taus=None):
        """Ground truths without an estimate: every threshold missed.  vsd_taus: how many tolerances the VSD entries carry (None:
        as many as the object's other entries, or no VSD entry when it has none)."""
        cor, _ = self._slot(obj_name)
        for e in ("mssd", "mspd"):
            cor[e] += [np.zeros(10, dtype=bool)] * count
        T = vsd_taus if vsd_taus is not None else (cor["vsd"][0].shape[1] if cor["vsd"] else 0)
        if T:
            cor["vsd"] += [np.zeros((10, T), dtype=bool)] * count

    def recalls(self, obj_name):
        """{"mssd": f[10], "mspd": f[10], "vsd": f[10] (mean over tau) or None, "AR_mssd", "AR_mspd", "AR_vsd" (or None), "AR"}."""
        cor = self.correct[obj_name]
        out = {}
        for e in ("mssd", "mspd", "vsd"):
            if cor[e]:
                a = np.stack(cor[e]).astype(np.float64)             # [instances, 10(, T)]
                out[e] = a.reshape(a.shape[0], 10, -1).mean(axis=(0, 2))
                out["AR_" + e] = float(a.mean())
            else:
                out[e], out["AR_" + e] = None, None
        ars = [out["AR_" + e] for e in ("mssd", "mspd", "vsd") if out["AR_" + e] is not None]
        out["AR"] = float(np.mean(ars)) if ars else 0.0
        return out

    def table(self):
        obj_names = sorted(self.correct.keys())
        rec = {o: self.recalls(o) for o in obj_names}
        errs = [e for e in ("mssd", "mspd", "vsd") if any(rec[o][e] is not None for o in obj_names)]
        rows = []
        for e in errs:
            thetas = BOP_MSPD_THETAS if e == "mspd" else BOP_THETAS
            rows += [("%s_%g" % (e, th), [None if rec[o][e] is None else rec[o][e][i] for o in obj_names]) for i, th in enumerate(thetas)]
            rows.append(("AR_" + e, [rec[o]["AR_" + e] for o in obj_names]))
        rows.append(("AR", [rec[o]["AR"] for o in obj_names]))
        tab = [["objects"] + obj_names + ["Avg(%d)" % len(obj_names)]]
        for name, vals in rows:
            have = [v for v in vals if v is not None]
            line = [name] + ["%.2f" % (100 * v) if v is not None else "-" for v in vals]
            if obj_names:
                line.append("%.2f" % (100 * np.mean(have)) if have else "-")
            tab.append(line)
        return tab

    def format(self):
        tab = [[str(c) for c in row] for row in self.table()]
        width = [max(len(r[i]) for r in tab if i < len(r)) for i in range(max(len(r) for r in tab))]
        return "\n".join("  ".join(c.ljust(width[i]) for i, c in enumerate(r)).rstrip() for r in tab)

    def dump(self, output_dir, dataset_name, method_name=""):
        """`{method}_{dataset}_bop_errors.pkl` (the per-instance errors) and `{method}_{dataset}_bop_tab.txt` beside RecallTable's."""
        import os
        import pickle
        os.makedirs(output_dir, exist_ok=True)
        stem = os.path.join(output_dir, "%s_%s" % (method_name, dataset_name))
        paths = (stem + "_bop_errors.pkl", stem + "_bop_tab.txt")
        with open(paths[0], "wb") as f:
            pickle.dump(self.errors, f)
        with open(paths[1], "w") as f:
            f.write("%s\n" % self.format())
        return paths
