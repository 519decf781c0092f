"""GPU: soft-assignment matching (csrc/gdm_match.hip match_panel_soft_kernel) and the weighted pose fit (csrc/gdm_pose.hip).

The soft launch must return the hard path's pairs bit for bit; lse / conf / soft_xyz are held to fp64 evaluations (a) over the
kernel's own similarities (ops.match(return_sim=True), bit-identical to what the soft kernel sees) with a bound from the fp32
accumulation alone, and (b) from the raw descriptors (matching.match_soft_numpy) with the project's similarity tolerance 1e-4
propagated through the softmax.  Every input comes from a seed."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

from geometric_aware_dense_matching_amd import matching, ops, pose, synthetic
from geometric_aware_dense_matching_amd.config import make_model_cfg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DELTA = 1e-4                                                            # the project's similarity tolerance
SHAPES = [(2, 70, 200), (1, 256, 256), (3, 128, 8193)]
GAMMAS = [16.0, 40.0]
SENTINEL = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -1000]], np.float32)


def _desc(rs, B, N, M):                                                 # as tests/test_gpu_ops.py::_desc
    scene = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32) * rs.rand(B, 1, N).astype(np.float32) * 3)
    model = torch.from_numpy(rs.randn(128, M).astype(np.float32))
    return scene, model


@functools.lru_cache(maxsize=None)
def _case(B, N, M, kind="random"):
    rs = np.random.RandomState(zlib.crc32(("match_soft %d %d %d %s" % (B, N, M, kind)).encode()))
    scene, model = _desc(rs, B, N, M)
    xyz = torch.from_numpy((0.05 * rs.uniform(-1, 1, (M, 3))).astype(np.float32))
    planted = None
    if kind == "ties":
        model[:, 300:] = model[:, :212]
    if kind == "planted":
        # the first and last column of every 32-column accumulator block of the one panel launched, and r mod M
        edges = [c for k in range(0, M, 32) for c in (k, min(k + 31, M - 1))]
        planted = np.array([edges[(r // 2) % len(edges)] if r % 2 == 0 else r % M for r in range(B * N)])
        scene = model[:, torch.from_numpy(planted)].reshape(128, B, N).permute(1, 0, 2).contiguous()
    return scene.cuda(), model.cuda(), xyz.cuda(), planted


@functools.lru_cache(maxsize=None)
def _soft(B, N, M, prec, gamma, kind="random"):
    scene, model, xyz, _ = _case(B, N, M, kind)
    srows, mrows = ops.match_pack2(scene, model, prec)
    out = ops.match_soft_packed(srows, mrows, xyz, B, N, M, prec, gamma)
    hard = ops.match_packed(srows, mrows, B, N, M, prec)
    torch.cuda.synchronize()
    return [t.clone() for t in out], [t.clone() for t in hard]


@functools.lru_cache(maxsize=None)
def _ref_from_sim(B, N, M, prec, gamma):
    scene, model, xyz, _ = _case(B, N, M)
    sim = ops.match(scene, model, prec, return_sim=True)[2].cpu().numpy().reshape(B * N, M)
    return matching.match_soft_numpy(sim, None, xyz.cpu().numpy(), gamma)


@functools.lru_cache(maxsize=None)
def _ref_from_descriptors(B, N, M, gamma, kind="random"):
    scene, model, xyz, _ = _case(B, N, M, kind)
    s, m, x = scene.cpu().numpy(), model.cpu().numpy(), xyz.cpu().numpy()
    parts = [matching.match_soft_numpy(s[b].T, m, x, gamma) for b in range(B)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _np(out):
    bi, bs, lse, conf, sxyz = [t.cpu().numpy() for t in out]
    return bi.reshape(-1), bs.reshape(-1), lse.reshape(-1).astype(np.float64), conf.reshape(-1).astype(np.float64), \
        sxyz.reshape(-1, 3).astype(np.float64)


# ---- 1: the hard path's pairs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_soft_launch_returns_the_hard_pairs(B, N, M, prec, gamma):
    """(2,70,200): a partial row block spanning two crops and a partial panel; (1,256,256): exactly one of each; (3,128,8193): 33
    panels, the last one column wide."""
    soft, hard = _soft(B, N, M, prec, gamma)
    assert torch.equal(soft[0], hard[0]) and torch.equal(soft[1], hard[1])
    assert all(bool(torch.isfinite(t).all()) for t in soft[1:])


@pytest.mark.parametrize("prec", [0, 1])
def test_exact_ties_take_the_first_maximum(prec):
    """Columns 300..511 repeat columns 0..211 bit for bit: the arg-max never lands on a copy, and a best vertex that has a copy
    cannot hold more than half of the probability."""
    soft, hard = _soft(1, 256, 512, prec, 16.0, "ties")
    assert torch.equal(soft[0], hard[0]) and torch.equal(soft[1], hard[1])
    bi, conf = soft[0].cpu().numpy().reshape(-1), soft[3].cpu().numpy().reshape(-1)
    assert (bi < 300).all() and (bi < 212).sum() >= 100
    assert (conf[bi < 212] <= 0.5).all() and (conf > 0).all()


@pytest.mark.parametrize("prec", [0, 1])
def test_conf_stays_in_its_range_when_one_column_dominates(prec):
    """conf = (the best column's own term of Z) / Z: exactly 1 with a single model column, never above 1 on a planted exact match at
    gamma = 40, and never above 0.5 when the planted column has a bit-identical copy."""
    scene, model, xyz, _ = _case(2, 70, 200, "planted")
    one = ops.match_soft(scene, model[:, :1].contiguous(), xyz[:1].contiguous(), prec, 40.0)
    assert bool((one[3] == 1).all()) and bool((one[0] == 0).all())
    c = (1 + 8 * 40 + 8) * U                                            # test 2's bounds at M = 1: lse64 = gamma sim, soft64 = xyz[0]
    assert bool(((one[2].double() - 40.0 * one[1].double()).abs() <= c + 4 * U * 40).all())
    assert bool(((one[4] - xyz[0]).abs() <= 2 * c * float(xyz[0].abs().max())).all())
    conf = ops.match_soft(scene, model, xyz, prec, 40.0)[3]
    assert bool((conf <= 1).all()) and bool((conf > 0.999).all())
    dup = torch.cat([model, model], dim=1)
    conf2 = ops.match_soft(scene, dup, torch.cat([xyz, xyz]), prec, 40.0)[3]
    assert bool((conf2 <= 0.5).all()) and bool((conf2 > 0.4995).all())


# ---- 2: fp64 over the kernel's own similarities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_soft_outputs_vs_fp64_over_the_kernels_similarities(B, N, M, prec, gamma):
    """c = (M + 8 gamma + 8) u: M fp32 additions of positive terms in any order, plus at most (8 gamma + 8) ulp per term from the
    exponent argument and exp2.  |lse - lse64| <= c + 4 u |lse64|, |conf - conf64| <= 2 c conf64 + u, |soft - soft64| <= 2 c max|xyz|."""
    bi, bs, lse, conf, sxyz = _np(_soft(B, N, M, prec, gamma)[0])
    ref = _ref_from_sim(B, N, M, prec, gamma)
    xmax = float(_case(B, N, M)[2].abs().max())
    c = (M + 8 * gamma + 8) * U
    assert np.array_equal(bi, ref["best_idx"]) and np.array_equal(bs.astype(np.float64), ref["best_sim"])
    e_lse = np.abs(lse - ref["lse"]) - 4 * U * np.abs(ref["lse"])
    e_conf = np.abs(conf - ref["conf"]) - 2 * c * ref["conf"]
    e_soft = np.abs(sxyz - ref["soft_xyz"]).max()
    print("lse excess %.3g of %.3g, conf excess %.3g of %.3g, soft %.3g of %.3g" % (e_lse.max(), c, e_conf.max(), U, e_soft, 2 * c * xmax))
    assert e_lse.max() <= c
    assert e_conf.max() <= U
    assert e_soft <= 2 * c * xmax


# ---- 3: the fp64 restatement from the descriptors ------------------------------------------------------------------------------------
def _check_vs_restatement(got, ref, gamma, xyz):
    bi, bs, lse, conf, sxyz = got
    E = np.expm1(2 * gamma * DELTA)
    rho = float(np.linalg.norm(xyz - xyz.mean(0), axis=1).max())
    e_lse = np.abs(lse - ref["lse"]).max()
    e_conf = (np.abs(conf - ref["conf"]) - E * ref["conf"]).max()
    e_soft = np.abs(sxyz - ref["soft_xyz"]).max()
    print("lse %.3g of %.3g, conf excess %.3g of 1e-6, soft %.3g of %.3g" % (e_lse, gamma * DELTA + 1e-5, e_conf, e_soft, E * rho + 1e-6))
    assert e_lse <= gamma * DELTA + 1e-5
    assert e_conf <= 1e-6
    assert e_soft <= E * rho + 1e-6
    return E, rho


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_soft_outputs_vs_fp64_restatement(B, N, M, prec, gamma):
    """Each similarity is within delta = 1e-4 of its fp64 value, so each weight moves by a factor within e^(+-gamma delta) and each
    probability by a factor within e^(+-2 gamma delta): with E = e^(2 gamma delta) - 1 and rho = max |xyz - centroid|,
    |lse - lse64| <= gamma delta + 1e-5, |conf - conf64| <= E conf64 + 1e-6, |soft - soft64|_inf <= E rho + 1e-6."""
    _check_vs_restatement(_np(_soft(B, N, M, prec, gamma)[0]), _ref_from_descriptors(B, N, M, gamma), gamma,
                          _case(B, N, M)[2].cpu().numpy().astype(np.float64))


# ---- 4: planted columns ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
def test_planted_columns(prec):
    """Scene row r is a copy of model column c_r; c_r walks over the first and last column of every accumulator block and over
    r mod M.  A dropped or doubled edge column fails this grossly: conf is close to 1 and soft_xyz close to xyz[c_r]."""
    B, N, M, gamma = 2, 70, 200, 16.0
    scene, model, xyz, planted = _case(B, N, M, "planted")
    got = _np(_soft(B, N, M, prec, gamma, "planted")[0])
    ref = _ref_from_descriptors(B, N, M, gamma, "planted")
    x = xyz.cpu().numpy().astype(np.float64)
    assert set(planted) >= {0, 31, 32, 63, 64, 127, 128, 191, 192, 199}
    assert np.array_equal(got[0], planted) and np.array_equal(ref["best_idx"], planted)
    E, rho = _check_vs_restatement(got, ref, gamma, x)
    assert ref["conf"].min() > 0.99
    d, d64 = np.linalg.norm(got[4] - x[planted], axis=1), np.linalg.norm(ref["soft_xyz"] - x[planted], axis=1)
    assert np.abs(d - d64).max() <= E * rho + 1e-6


# ---- 5: repeatability ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
def test_two_launches_are_bit_identical(prec):
    B, N, M = 3, 128, 8193
    scene, model, xyz, _ = _case(B, N, M)
    first = _soft(B, N, M, prec, 16.0)[0]
    again = ops.match_soft(scene, model, xyz, prec, 16.0)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


# ---- 6: weighted statistics and fit ----------------------------------------------------------------------------------------------------
def _rotation(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def _fit_case():
    B, N, M = 4, 70, 200
    rs = np.random.RandomState(zlib.crc32(b"weighted fit"))
    model = (0.05 * rs.uniform(-1, 1, (M, 3))).astype(np.float32)
    idx = rs.randint(0, M, (B, N)).astype(np.int32)
    target = (model[idx] + rs.randn(B, N, 3) * 1e-3).astype(np.float32)
    cld = rs.rand(B, 9, N).astype(np.float32)
    for b in range(B):
        R, t = _rotation(rs), np.array([0.1 * rs.randn(), 0.1 * rs.randn(), 0.7])
        cld[b, :3] = (model[idx[b]].astype(np.float64) @ R.T + t + rs.randn(N, 3) * 1e-3).T
    mask = (rs.rand(B, N) < 0.6).astype(np.uint8)
    mask[1] = 0
    mask[1, [3, 17, 40, 69]] = 1                                        # four points: below min_points
    w = rs.rand(B, N).astype(np.float32) + 0.01
    w[2] = 0                                                            # no weight at all
    bad = np.nonzero(mask[3])[0][::4]
    w[3, bad] = np.array([np.nan, -1.0, np.inf, 0.0], np.float32)[np.arange(len(bad)) % 4]
    return model, idx, target, cld, mask, w


def _weighted_ref(model, idx, target, cld, mask, w, use_target):
    B = mask.shape[0]
    want, mag, count, RT = np.zeros((B, 16)), np.zeros((B, 16)), np.zeros(B, np.int32), [None] * B
    for b in range(B):
        sel = (mask[b] != 0) & np.isfinite(w[b]) & (w[b] > 0)
        A = (target[b] if use_target else model[idx[b]])[sel].astype(np.float64)
        P = cld[b, :3].T[sel].astype(np.float64)
        ww = w[b][sel].astype(np.float64)
        terms = ww[:, None] * np.concatenate([np.ones((len(A), 1)), A, P, (A[:, :, None] * P[:, None, :]).reshape(-1, 9)], axis=1)
        want[b], mag[b], count[b] = terms.sum(0), np.abs(terms).sum(0), sel.sum()
        if count[b] >= 5 and ww.sum() > 0:
            RT[b] = pose.kabsch_weighted_numpy(A, P, ww)
    return want, mag, count, RT


@pytest.mark.parametrize("targets", ["vertex", "soft"])
def test_weighted_statistics_and_fit(targets):
    """Crop 0 ordinary, crop 1 with four masked points, crop 2 with every weight 0, crop 3 with NaN / negative / infinite / zero
    weights among good ones.  Statistics to 1e-12 of the sum of the terms' magnitudes and the count exactly (the rule of
    tests/test_gpu_pose_shapes.py), RT to that file's bounds for a unique fit (R 1e-7, t one fp32 ulp of max(1, |t|))."""
    model, idx, target, cld, mask, w = _fit_case()
    use_target = targets == "soft"
    want, mag, count, RTw = _weighted_ref(model, idx, target, cld, mask, w, use_target)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    res = dict(mask=c(mask), best_idx=c(idx), conf=c(w), soft_xyz=c(target))
    st, cnt = pose.kabsch_stats_weighted(res, c(cld), c(model), res["conf"], c(target) if use_target else None)
    assert np.array_equal(cnt.cpu().numpy(), count) and count[1] == 4 and count[2] == 0 and 5 <= count[3] < mask[3].sum()
    err = np.abs(st.cpu().numpy() - want)
    assert (err <= 1e-12 * mag).all(), float((err - 1e-12 * mag).max())
    if not use_target:
        del res["soft_xyz"]                                             # weights="conf" with vertex targets reads conf only
    RT, valid = pose.solve_poses(res, c(cld), c(model), weights="conf", targets=targets)
    RT2, valid2 = pose.solve_poses_weighted(res, c(cld), c(model), res["conf"], c(target) if use_target else None)
    assert torch.equal(RT, RT2) and torch.equal(valid, valid2)
    RT, valid = RT.cpu().numpy(), valid.cpu().numpy()
    assert valid.tolist() == [True, False, False, True]
    for b in range(4):
        if not valid[b]:
            assert np.array_equal(RT[b], SENTINEL), b
            continue
        assert np.abs(RT[b, :, :3] - RTw[b][:, :3]).max() <= 1e-7, (b, float(np.abs(RT[b, :, :3] - RTw[b][:, :3]).max()))
        tol = 2.0 ** -23 * max(1.0, float(np.abs(RTw[b][:, 3]).max()))
        assert np.abs(RT[b, :, 3] - RTw[b][:, 3]).max() <= tol, b


def test_unit_weights_reproduce_the_unweighted_fit_bit_for_bit():
    model, idx, target, cld, mask, w = _fit_case()
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    res = dict(mask=c(mask), best_idx=c(idx))
    RT, valid = pose.solve_poses(res, c(cld), c(model))
    RTw, validw = pose.solve_poses_weighted(res, c(cld), c(model), torch.ones(mask.shape, device="cuda"))
    assert torch.equal(RT, RTw) and torch.equal(valid, validw) and valid.tolist() == [True, False, True, True]
    st, cnt = pose.kabsch_stats_weighted(res, c(cld), c(model), torch.ones(mask.shape, device="cuda"))
    assert torch.equal(st, pose.kabsch_stats(res, c(cld), c(model))) and np.array_equal(cnt.cpu().numpy(), (mask != 0).sum(1))


# ---- 7: the pipeline -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1_model():
    """The C1 model of tests/test_gpu_model.py: M = 512 mesh vertices, the committed key list, seeded weights."""
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    M = 512
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "geomatch_state.json")))
    sd = synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def _inputs(seed):
    batch = synthetic.make_batch(seed=seed, batch=1, n_points=1024)
    return {k: torch.from_numpy(batch[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}


SOFT_KW = dict(with_pose=True, match_gamma=16.0, pose_opts=dict(weights="conf", targets="soft"))


def _check_score(out):
    conf, mask = out["conf"].cpu().numpy().astype(np.float64), out["mask"].cpu().numpy() != 0
    want = np.array([conf[b][mask[b]].mean() if mask[b].any() else 0.0 for b in range(len(conf))])
    assert np.abs(out["score"].cpu().numpy() - want).max() <= 2.0 ** -24          # one rounding of an fp64 mean in [0, 1]


def test_pipeline_step_with_soft_matching(c1_model):
    from geometric_aware_dense_matching_amd import infer
    model, d = c1_model, _inputs(61)
    with torch.no_grad():
        base = infer.pipeline_step(model, d, with_pose=True)
        same = infer.pipeline_step(model, d, with_pose=True, match_gamma=None)
        soft = infer.pipeline_step(model, d, **SOFT_KW)
        direct = ops.match_soft(soft["rgbd"], soft["mesh"], model.model_emb.xyz, ops.MATCH_BF16X3, 16.0)
        RT, valid = pose.solve_poses(soft, d["cld_rgb_nrm"], model.model_emb.xyz, weights="conf", targets="soft")
    ok, bad = infer.outputs_equal(base, same)
    assert ok and set(base) == set(same), bad
    assert set(soft) == set(base) | {"lse", "conf", "soft_xyz", "score"}
    for k in base:
        if k not in ("RT", "valid"):
            assert torch.equal(base[k], soft[k]), k
    for k, t in zip(("best_idx", "best_sim", "lse", "conf", "soft_xyz"), direct):
        assert torch.equal(soft[k], t), k
    assert torch.equal(soft["RT"], RT) and torch.equal(soft["valid"], valid)
    assert soft["score"].shape == (1,)
    _check_score(soft)


def test_graphed_pipeline_with_soft_matching_replays_the_eager_step(c1_model):
    from geometric_aware_dense_matching_amd import infer
    model = c1_model
    gp = infer.GraphedPipeline(model, _inputs(61), forked=False, **SOFT_KW)
    assert gp.form == "single" and gp.check["single"]["bit_identical"], gp.check
    for seed in (62, 63, 64):
        d = _inputs(seed)
        got = {k: v.clone() for k, v in gp(d).items()}
        with torch.no_grad():
            want = infer.pipeline_step(model, d, **SOFT_KW)
        ok, bad = infer.outputs_equal(want, got)
        assert ok and set(want) == set(got) and "score" in got, (seed, bad)
        _check_score(got)


def test_run_multi_object_and_test_entry_point_with_soft_matching(c1_model, tmp_path):
    """run_multi_object(match_gamma=...) concatenates the soft outputs and the score per instance like the rest, and equals the
    batched pipeline_step on the same crops; `train_lm.py -state=test --match-gamma 16 --pose-weights conf --pose-targets soft
    --eval-output DIR` runs and writes each instance's score into the BOP csv."""
    from geometric_aware_dense_matching_amd import infer, train_lm
    batch = synthetic.make_batch(seed=71, batch=3, n_points=1024)
    d = {k: torch.from_numpy(batch[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
    kw = dict(match_gamma=16.0, pose_opts=dict(weights="conf", targets="soft"))
    out = infer.run_multi_object({1: c1_model}, d, [1, 1, 1], **kw)
    assert out["score"].shape == (3,) and out["conf"].shape == (3, 1024) and out["soft_xyz"].shape == (3, 1024, 3)
    _check_score(out)
    with torch.no_grad():
        want = infer.pipeline_step(c1_model, d, with_pose=True, **kw)
    for k in ("best_idx", "best_sim", "lse", "conf", "soft_xyz", "score", "RT", "valid"):
        assert torch.equal(out[k], want[k]), k
    with pytest.raises(ValueError, match="RANSAC keeps the hard pairs"):
        infer.run_multi_object({1: c1_model}, d, [1, 1, 1], pose_fit="ransac", **kw)
    argv = ("--gpus=0 -state=test -cls_id=1 --single-object --batch-size 2 --n-points 1024 --n-mesh 512 --synthetic-items 4 "
            "--match-gamma 16 --pose-weights conf --pose-targets soft --eval-output %s" % tmp_path).split()
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    assert len(res) == 2
    csv = [p for p in train_lm.test.last_outputs if p.endswith("-test.csv")]
    lines = open(csv[0]).read().split("\n")
    scores = [float(ln.split(",")[3]) for ln in lines[1:]]
    assert len(scores) == 4 and scores == [float(s) for r in res for s in r["score"]]
    for r in res:
        m = r["mask"].numpy() != 0
        mean = [r["conf"][b].double().numpy()[m[b]].mean() if m[b].any() else 0.0 for b in range(len(m))]
        assert np.abs(r["score"].numpy() - np.array(mean)).max() <= 2.0 ** -24
    plain = train_lm.test(train_lm.build_parser().parse_args(argv[:argv.index("--match-gamma")] + argv[-2:]))
    assert "score" not in plain[0] and all(ln.split(",")[3] == "-1" for ln in open(csv[0]).read().split("\n")[1:])
