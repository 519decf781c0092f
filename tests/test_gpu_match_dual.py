"""GPU: dual-softmax matching (csrc/gdm_match.hip match_panel_dual_kernel, dual_cols_kernel, dual_rows_kernel).

The dual launch must return the soft launch's five row outputs and the two-way launch's two column outputs bit for bit.  col_lse,
col_conf and dual are held to fp64 evaluations (a) over the kernel's own similarities (ops.match(return_sim=True), bit-identical to
what the kernel sees, as tests/test_gpu_match_soft.py relies on) with a bound from the fp32 accumulation alone, and (b) from the raw
descriptors (matching.match_dual_numpy) with the project's similarity tolerance 1e-4 propagated through both softmaxes.  Inputs:
tests/match_twoway_cases.py (descriptors) and tests/match_dual_cases.py (shapes, masks, vertices)."""
import functools

import numpy as np
import pytest
import torch

import match_dual_cases as dc
import match_twoway_cases as mc
from geometric_aware_dense_matching_amd import _lib, infer, matching, ops, pose

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DELTA = 1e-4                                                            # the project's similarity tolerance
ROWS = ("best_idx", "best_sim", "lse", "conf", "soft_xyz")
CASES = [pytest.param(B, N, M, id="%dx%dx%d" % (B, N, M)) for B, N, M in dc.SHAPES]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(B, N, M):
    scene, model = mc.descriptors(B, N, M)
    return _cuda(scene), _cuda(model), _cuda(dc.model_xyz(M))


@functools.lru_cache(maxsize=None)
def _rows(B, N, M, prec):
    scene, model, _ = _case(B, N, M)
    return ops.match_pack2(scene, model, prec)


@functools.lru_cache(maxsize=None)
def _dual(B, N, M, prec, gamma, kind):
    srows, mrows = _rows(B, N, M, prec)
    out = ops.match_dual_packed(srows, mrows, _case(B, N, M)[2], _cuda(dc.mask(B, N, kind)), B, N, M, prec, gamma)
    torch.cuda.synchronize()
    return dict(zip(ops.DUAL_KEYS, [t.clone() for t in out]))


@functools.lru_cache(maxsize=None)
def _soft(B, N, M, prec, gamma):
    srows, mrows = _rows(B, N, M, prec)
    return [t.clone() for t in ops.match_soft_packed(srows, mrows, _case(B, N, M)[2], B, N, M, prec, gamma)]


@functools.lru_cache(maxsize=None)
def _twoway(B, N, M, prec, kind):
    srows, mrows = _rows(B, N, M, prec)
    return [t.clone() for t in ops.match_twoway_packed(srows, mrows, _cuda(dc.mask(B, N, kind)), B, N, M, prec)]


@functools.lru_cache(maxsize=None)
def _sim(B, N, M, prec):
    """The kernel's own similarities, f32[B,N,M] on the host."""
    scene, model, _ = _case(B, N, M)
    return ops.match(scene, model, prec, return_sim=True)[2].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref_from_sim(B, N, M, prec, gamma, kind):
    sim, mask, xyz = _sim(B, N, M, prec), dc.mask(B, N, kind), dc.model_xyz(M)
    return [matching.match_dual_numpy(sim[b], None, xyz, mask[b], gamma) for b in range(B)]


@functools.lru_cache(maxsize=None)
def _sim64(B, N, M):
    """The fp64 similarities from the raw descriptors, normalised as matching.match_dual_numpy normalises them: [B][N,M]."""
    scene, model = mc.descriptors(B, N, M)
    b = model.astype(np.float64)
    b = b / np.maximum(np.linalg.norm(b, axis=0, keepdims=True), 1e-12)
    out = []
    for s in scene:
        a = s.T.astype(np.float64)
        out.append((a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)) @ b)
    return out


@functools.lru_cache(maxsize=None)
def _ref_from_descriptors(B, N, M, gamma, kind):
    mask, xyz = dc.mask(B, N, kind), dc.model_xyz(M)
    return [matching.match_dual_numpy(s, None, xyz, mask[b], gamma) for b, s in enumerate(_sim64(B, N, M))]


def _np64(d, k):
    return d[k].cpu().numpy().astype(np.float64)


# ---- 1: the soft launch's rows and the two-way launch's columns, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("kind", dc.MASKS)
@pytest.mark.parametrize("gamma", dc.GAMMAS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", CASES)
def test_dual_launch_returns_the_soft_rows_and_the_twoway_columns(B, N, M, prec, gamma, kind):
    """The dual kernel cuts the rows crop by crop, the other two kernels in blocks of 256 over the whole batch: a row sits in another
    wave, lane and register, and its outputs must not notice.  Every row, masked or not; every column of every crop."""
    d, soft, two = _dual(B, N, M, prec, gamma, kind), _soft(B, N, M, prec, gamma), _twoway(B, N, M, prec, kind)
    for k, t in zip(ROWS, soft):
        assert d[k].dtype == t.dtype and torch.equal(d[k].view(torch.int32), t.view(torch.int32)), k
    assert torch.equal(d["best_idx"], two[0]) and torch.equal(d["best_sim"].view(torch.int32), two[1].view(torch.int32))
    assert torch.equal(d["col_idx"], two[2]) and torch.equal(d["col_sim"].view(torch.int32), two[3].view(torch.int32))
    for k in ("col_lse", "col_conf"):
        assert d[k].shape == (B, M) and d[k].dtype == torch.float32
    assert d["dual"].shape == (B, N) and d["dual"].dtype == torch.float32


# ---- 2: fp64 over the kernel's own similarities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dc.MASKS)
@pytest.mark.parametrize("gamma", dc.GAMMAS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", CASES)
def test_dual_outputs_vs_fp64_over_the_kernels_similarities(B, N, M, prec, gamma, kind):
    """tests/test_gpu_match_soft.py test 2 with the masked count n of the crop in place of M: cc = (n + 8 gamma + 8) u bounds the
    relative error of Zc (n fp32 additions of positive terms in any order, at most (8 gamma + 8) ulp per term from the exponent
    argument and exp2), so |col_lse - ref| <= cc + 4 u |ref| and |col_conf - ref| <= 2 cc ref + u.  dual = conf * q: conf is within
    2 cr conf64 + u of its fp64 value (cr = (M + 8 gamma + 8) u, that test's bound), q = w / Zc within 2 cc q64, so the product is
    within ((1 + 2 cr)(1 + 2 cc) - 1) ref = (2 (cr + cc) + 4 cr cc) ref, plus u from conf's absolute term (q <= 1) and u from the
    final rounding (dual <= 1): |dual - ref| <= (2 (cr + cc) + 4 cr cc) ref + 2 u."""
    d = _dual(B, N, M, prec, gamma, kind)
    mask = dc.mask(B, N, kind)
    cr = (M + 8 * gamma + 8) * U
    worst = dict(col_lse=-np.inf, col_conf=-np.inf, dual=-np.inf)
    for b, ref in enumerate(_ref_from_sim(B, N, M, prec, gamma, kind)):
        n = int((mask[b] != 0).sum())
        cc = (n + 8 * gamma + 8) * U
        col_lse, col_conf, dual = _np64(d, "col_lse")[b], _np64(d, "col_conf")[b], _np64(d, "dual")[b]
        assert np.array_equal(d["col_idx"][b].cpu().numpy(), ref["col_idx"])
        if n == 0:
            assert np.isneginf(col_lse).all() and (col_conf == 0).all() and (dual == 0).all()
            continue
        e_lse = (np.abs(col_lse - ref["col_lse"]) - 4 * U * np.abs(ref["col_lse"])).max() - cc
        e_conf = (np.abs(col_conf - ref["col_conf"]) - 2 * cc * ref["col_conf"]).max() - U
        e_dual = (np.abs(dual - ref["dual"]) - (2 * (cr + cc) + 4 * cr * cc) * ref["dual"]).max() - 2 * U
        for k, e in (("col_lse", e_lse), ("col_conf", e_conf), ("dual", e_dual)):
            worst[k] = max(worst[k], float(e))
    print("excess over the bound (<= 0 passes): col_lse %.3g, col_conf %.3g, dual %.3g" % (worst["col_lse"], worst["col_conf"], worst["dual"]))
    assert worst["col_lse"] <= 0 and worst["col_conf"] <= 0 and worst["dual"] <= 0


# ---- 3: the fp64 restatement from the descriptors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dc.MASKS)
@pytest.mark.parametrize("gamma", dc.GAMMAS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", CASES)
def test_dual_outputs_vs_fp64_restatement(B, N, M, prec, gamma, kind):
    """Each similarity is within delta = 1e-4 of its fp64 value, so every weight moves by a factor within e^(+-gamma delta), every
    column sum too, a share of a row or of a column by e^(+-2 gamma delta) and their product by e^(+-4 gamma delta):
    |col_lse - ref| <= gamma delta + 1e-5, |col_conf - ref| <= E2 ref + 1e-6, |dual - ref| <= E4 ref + 1e-6 (the absolute terms as
    in tests/test_gpu_match_soft.py test 3).  Two similarities within 2 delta of each other may swap their order, so the fp64 dual
    is taken at the vertex the kernel names (whose fp64 similarity the kernel's best_sim is within delta of); col_conf needs no such
    care, it depends on the value of the column's maximum alone."""
    d = _dual(B, N, M, prec, gamma, kind)
    mask = dc.mask(B, N, kind)
    E2, E4 = np.expm1(2 * gamma * DELTA), np.expm1(4 * gamma * DELTA)
    worst = [-np.inf] * 3
    for b, (ref, s64) in enumerate(zip(_ref_from_descriptors(B, N, M, gamma, kind), _sim64(B, N, M))):
        keep = mask[b] != 0
        if not keep.any():
            assert np.isneginf(_np64(d, "col_lse")[b]).all() and np.isneginf(ref["col_lse"]).all()
            continue
        j = d["best_idx"][b].cpu().numpy().astype(np.int64)
        assert (np.abs(s64[np.arange(N), j] - _np64(d, "best_sim")[b]) <= DELTA).all()
        want = np.where(keep, ref["conf"] * np.exp(gamma * s64[np.arange(N), j] - ref["col_lse"][j]), 0.0)
        same = j == ref["best_idx"]
        assert np.array_equal(want[same], ref["dual"][same])              # where the arg-max agrees this is the restatement's own dual
        worst[0] = max(worst[0], float(np.abs(_np64(d, "col_lse")[b] - ref["col_lse"]).max() - gamma * DELTA - 1e-5))
        worst[1] = max(worst[1], float((np.abs(_np64(d, "col_conf")[b] - ref["col_conf"]) - E2 * ref["col_conf"]).max() - 1e-6))
        worst[2] = max(worst[2], float((np.abs(_np64(d, "dual")[b] - want) - E4 * want).max() - 1e-6))
    print("excess over the bound (<= 0 passes): col_lse %.3g, col_conf %.3g, dual %.3g" % tuple(worst))
    assert max(worst) <= 0


# ---- 4: ranges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dc.MASKS)
@pytest.mark.parametrize("gamma", dc.GAMMAS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", CASES)
def test_ranges_hold_everywhere(B, N, M, prec, gamma, kind):
    d = {k: v.cpu().numpy() for k, v in _dual(B, N, M, prec, gamma, kind).items()}
    mask = dc.mask(B, N, kind) != 0
    assert (d["dual"] >= 0).all() and (d["dual"] <= d["conf"]).all() and (d["conf"] <= 1).all()
    assert (d["dual"][~mask] == 0).all() and (d["dual"][mask] > 0).all()
    has = d["col_idx"] >= 0
    assert np.array_equal(has, np.broadcast_to(mask.any(axis=1)[:, None], has.shape))
    assert (d["col_conf"][has] > 0).all() and (d["col_conf"][has] <= 1).all() and (d["col_conf"][~has] == 0).all()
    assert np.isneginf(d["col_lse"][~has]).all() and np.isfinite(d["col_lse"][has]).all()
    for b in np.flatnonzero(mask.sum(axis=1) == 1):                        # one masked point: the only term of every column
        i = int(np.flatnonzero(mask[b])[0])
        assert (d["col_conf"][b] == 1).all() and (d["col_idx"][b] == i).all()
        assert d["dual"][b, i].tobytes() == d["conf"][b, i].tobytes()


@pytest.mark.parametrize("prec", [0, 1])
def test_a_duplicated_point_holds_at_most_half_of_its_column(prec):
    """Scene points 3 and 200 of crop 0 are bit-identical copies of model column 17 (they sit in different waves): both masked,
    vertex 17 names the lower one, its column share is at most 0.5, and so is dual / conf of either point."""
    B, N, M = 2, 300, 256
    scene, model = mc.descriptors(B, N, M)
    scene = scene.copy()
    scene[0][:, 3] = scene[0][:, 200] = model[:, 17]
    for gamma in dc.GAMMAS:
        out = dict(zip(ops.DUAL_KEYS, ops.match_dual(_cuda(scene), _cuda(model), _cuda(dc.model_xyz(M)),
                                                     torch.ones(B, N, dtype=torch.uint8, device="cuda"), prec, gamma)))
        assert int(out["best_idx"][0, 3]) == 17 and int(out["best_idx"][0, 200]) == 17 and int(out["col_idx"][0, 17]) == 3
        share = float(out["col_conf"][0, 17])
        print("gamma %g: col_conf %.6f" % (gamma, share))
        assert 0 < share <= 0.5
        for i in (3, 200):
            assert torch.equal(out["dual"][0, i], out["dual"][0, 3]) and float(out["dual"][0, i]) <= 0.5 * float(out["conf"][0, i])


# ---- 5: the same bytes on every launch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", [(2, 300, 256), (5, 20, 300), (3, 128, 8193)])
def test_two_launches_and_a_dirty_workspace_give_the_same_bytes(B, N, M, prec):
    srows, mrows = _rows(B, N, M, prec)
    xyz, mask = _case(B, N, M)[2], _cuda(dc.mask(B, N, "half"))
    nbytes = _lib.lib().gdm_match_dual_partial_bytes(B, N, M)
    pool = ops.BufferPool()
    with ops.buffer_pool(pool):
        first = [t.clone() for t in ops.match_dual_packed(srows, mrows, xyz, mask, B, N, M, prec, 16.0)]
        second = [t.clone() for t in ops.match_dual_packed(srows, mrows, xyz, mask, B, N, M, prec, 16.0)]
        ws = ops._workspace(nbytes, srows.device)
        ws.fill_(0xFF)
        third = ops.match_dual_packed(srows, mrows, xyz, mask, B, N, M, prec, 16.0)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), c.view(torch.uint8))
    L = _lib.lib()
    assert nbytes >= L.gdm_match_soft_partial_bytes(B, N) + 8 * B * M + 4 * B * ((N + 255) // 256) * M + 4 * B * M


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    B, N, M = 2, 70, 200
    srows, mrows = _rows(B, N, M, 0)
    xyz, mask = _case(B, N, M)[2], _cuda(dc.mask(B, N, "ones"))
    L = _lib.lib()

    def refused(match, s=srows, m=mrows, x=xyz, msk=mask, M_=M, prec=0, N_=N, gamma=16.0):
        f32, i32 = torch.float32, torch.int32
        o = [torch.full(shape, 7, dtype=dt, device="cuda") for shape, dt in
             (((B, N), i32), ((B, N), f32), ((B, N), f32), ((B, N), f32), ((B, N, 3), f32),
              ((B, M_), i32), ((B, M_), f32), ((B, M_), f32), ((B, M_), f32), ((B, N), f32))]
        part = torch.zeros(max(L.gdm_match_dual_partial_bytes(B, N, M_), 16), dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.GdmError, match=match):
            _lib.call("gdm_match_dual_packed_hip", s, m, x, msk, B, N_, M_, prec, gamma, *o, part, part.numel())
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in o) and not bool(part.any())

    big = torch.zeros(L.gdm_match_rows_bytes(16385), dtype=torch.uint8, device="cuda")
    refused(r"rc=-1.*M=16385", m=big, x=torch.zeros(16385, 3, device="cuda"), M_=16385)
    refused(r"rc=-1.*NULL", msk=None)
    refused(r"rc=-1.*NULL", x=None)
    off = torch.zeros(srows.numel() + 16, dtype=torch.uint8, device="cuda")
    refused(r"rc=-1.*16-byte aligned", s=off[4:4 + srows.numel()])
    refused(r"rc=-1.*16-byte aligned", m=off[4:4 + mrows.numel()])
    refused(r"rc=-1.*precision=2", prec=2)
    refused(r"rc=-1.*bad shape", N_=0)
    for gamma in (0.0, -1.0, 40.5, float("nan")):
        refused(r"rc=-1.*gamma", gamma=gamma)
    ep = dict(seg=torch.zeros(B, 2, N, device="cuda"), rgbd=_case(B, N, M)[0], mesh=_case(B, N, M)[1])
    with pytest.raises(ValueError, match="dual=True needs soft"):
        matching.match_frames(ep, dual=True)
    with pytest.raises(ValueError, match="do not pass twoway=True"):
        matching.match_frames(ep, soft=dict(gamma=16.0, model_xyz=xyz), twoway=True, dual=True)
    with pytest.raises(ValueError, match="mask is"):
        ops.match_dual_packed(srows, mrows, xyz, mask[:, :N - 1], B, N, M, 0, 16.0)


# ---- 7: the weighted fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
def test_dual_weights_are_the_weighted_fit_with_dual_as_the_weight(prec):
    """match_frames(soft=..., dual=True) on the planted inlier / outlier scene of the two-way tests; solve_poses(weights="dual") is
    solve_poses_weighted with res["dual"], bit for bit, also behind the cycle filter and with soft targets, and differs from the
    fit weighted by conf."""
    c = mc.filter_case()
    B, _, N = c["scene"].shape
    cld, xyz = _cuda(c["cld"]), _cuda(c["model_xyz"])
    seg = torch.zeros(B, 2, N, device="cuda")
    seg[:, 1] = 1                                                          # every point is on the object
    ep = dict(seg=seg, rgbd=_cuda(c["scene"]), mesh=_cuda(c["model"])[None])
    res = matching.match_frames(ep, precision=prec, soft=dict(gamma=16.0, model_xyz=xyz), dual=True)
    assert set(res) == {"mask", "count"} | set(ops.DUAL_KEYS) and bool(res["mask"].all())
    RT, valid = pose.solve_poses(res, cld, xyz, weights="dual")
    wRT, wvalid = pose.solve_poses_weighted(res, cld, xyz, res["dual"], None, 5)
    assert torch.equal(RT, wRT) and torch.equal(valid, wvalid) and bool(valid.all())
    cRT, _ = pose.solve_poses(res, cld, xyz, weights="conf")
    assert not torch.equal(RT, cRT)
    sRT, _ = pose.solve_poses(res, cld, xyz, weights="dual", targets="soft")
    assert torch.equal(sRT, pose.solve_poses_weighted(res, cld, xyz, res["dual"], res["soft_xyz"], 5)[0])
    # pair_filter="cycle" works on the dual result as it is: col_idx is there
    got = pose.estimate_poses(res, cld, xyz, pose_opts=dict(pair_filter="cycle", weights="dual"))
    pm, pc, _ = pose.cycle_filter(res, cld, pose.CYCLE_RADIUS)
    assert torch.equal(got["pair_mask"], pm) and torch.equal(pm, _cuda(c["inlier"]))
    assert torch.equal(got["RT"], pose.solve_poses_weighted(dict(res, mask=pm), cld, xyz, res["dual"], None, 5)[0])
    with pytest.raises(ValueError, match=r"need the soft matching outputs \['dual'\]"):
        pose.solve_poses({k: v for k, v in res.items() if k != "dual"}, cld, xyz, weights="dual")


# ---- 8: the pipeline --------------------------------------------------------------------------------------------------------------------
from test_gpu_match_soft import _inputs, c1_model          # noqa: E402,F401  (the C1 model fixture and its seeded crops)

DUAL_KW = dict(with_pose=True, match_gamma=16.0, match_dual=True, pose_opts=dict(pair_filter="cycle"))


def test_pipeline_step_with_dual_matching(c1_model):          # noqa: F811
    model, d = c1_model, _inputs(61)
    with torch.no_grad():
        base = infer.pipeline_step(model, d, with_pose=True)
        off = infer.pipeline_step(model, d, with_pose=True, match_dual=False)
        soft = infer.pipeline_step(model, d, with_pose=True, match_gamma=16.0)
        dual = infer.pipeline_step(model, d, **DUAL_KW)
        wdual = infer.pipeline_step(model, d, with_pose=True, match_gamma=16.0, match_dual=True, pose_opts=dict(weights="dual"))
        direct = ops.match_dual(dual["rgbd"], dual["mesh"], model.model_emb.xyz, dual["mask"], ops.MATCH_BF16X3, 16.0)
        pm, pc, _ = pose.cycle_filter(dual, d["cld_rgb_nrm"], pose.CYCLE_RADIUS)
        RT, valid = pose.solve_poses(dict(dual, mask=pm), d["cld_rgb_nrm"], model.model_emb.xyz)
        wRT, _ = pose.solve_poses(wdual, d["cld_rgb_nrm"], model.model_emb.xyz, weights="dual")
    ok, bad = infer.outputs_equal(base, off)
    assert ok and set(base) == set(off), bad                                     # off: what it was
    assert set(dual) == set(soft) | {"col_idx", "col_sim", "col_lse", "col_conf", "dual", "pair_mask", "pair_count"}
    for k in soft:
        if k not in ("RT", "valid"):
            assert torch.equal(soft[k], dual[k]), k                               # the soft step's outputs, the score included
    for k, t in zip(ops.DUAL_KEYS, direct):
        assert torch.equal(dual[k], t), k
    assert torch.equal(dual["pair_mask"], pm) and torch.equal(dual["pair_count"], pc)
    assert torch.equal(dual["RT"], RT) and torch.equal(dual["valid"], valid)
    assert torch.equal(wdual["RT"], wRT) and "pair_mask" not in wdual
    with pytest.raises(ValueError, match="twoway and soft exclude each other"):    # without match_dual today's refusal stands
        infer.pipeline_step(model, d, with_pose=True, match_gamma=16.0, pose_opts=dict(pair_filter="cycle"))


def test_graphed_pipeline_with_dual_matching_replays_the_eager_step(c1_model):          # noqa: F811
    model = c1_model
    gp = infer.GraphedPipeline(model, _inputs(61), forked=False, **DUAL_KW)
    assert gp.form == "single" and gp.check["single"]["bit_identical"], gp.check
    for seed in (62, 63):
        d = _inputs(seed)
        got = {k: v.clone() for k, v in gp(d).items()}
        with torch.no_grad():
            want = infer.pipeline_step(model, d, **DUAL_KW)
        ok, bad = infer.outputs_equal(want, got)
        assert ok and set(want) == set(got) and "dual" in got and "pair_count" in got, (seed, bad)


def test_run_multi_object_and_test_entry_point_with_dual_matching(c1_model, tmp_path):          # noqa: F811
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    batch = synthetic.make_batch(seed=71, batch=3, n_points=1024)
    d = {k: torch.from_numpy(batch[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
    kw = dict(match_gamma=16.0, match_dual=True, pose_opts=dict(pair_filter="cycle", weights="dual"))
    out = infer.run_multi_object({1: c1_model}, d, [1, 1, 1], **kw)
    with torch.no_grad():
        want = infer.pipeline_step(c1_model, d, with_pose=True, **kw)
    for k in ops.DUAL_KEYS + ("score", "pair_mask", "pair_count", "RT", "valid"):
        assert torch.equal(out[k], want[k]), k
    argv = ("--gpus=0 -state=test -cls_id=1 --single-object --batch-size 2 --n-points 1024 --n-mesh 512 --synthetic-items 4 "
            "--match-gamma 16 --match-dual --pose-weights dual --pair-filter cycle --match-score dual --eval-output %s" % tmp_path).split()
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    assert len(res) == 2 and all("pair_count" in r for r in res)
    csv = [p for p in train_lm.test.last_outputs if p.endswith("-test.csv")]
    scores = [float(ln.split(",")[3]) for ln in open(csv[0]).read().split("\n")[1:]]
    assert len(scores) == 4 and scores == [float(s) for r in res for s in r["score"]]
    by_conf = train_lm.test(train_lm.build_parser().parse_args(argv[:argv.index("--match-score")] + argv[-2:]))
    for key, runs in (("dual", res), ("conf", by_conf)):                             # each run's score: the mean of what it was asked for
        for r in runs:                                                               # (two runs of the entry point do not share their weights)
            m = r["mask"].numpy() != 0
            mean = [r[key][b].double().numpy()[m[b]].mean() if m[b].any() else 0.0 for b in range(len(m))]
            assert np.abs(r["score"].numpy() - np.array(mean)).max() <= 2.0 ** -24, key
            assert bool((r["dual"] <= r["conf"]).all())
    # the same two scores on crops that have masked points: the C1 model's
    assert int(out["mask"].sum()) > 0
    by_dual = ops.match_score(out["dual"], out["mask"])
    assert bool((by_dual <= out["score"]).all()) and not torch.equal(by_dual, out["score"])


# ---- 9: stream ordering -----------------------------------------------------------------------------------------------------------------
def test_forked_step_with_dual_matching_is_ordered():
    """tests/stream_audit.py takes the dual step as it is: the forked step audited as tests/test_gpu_stream_audit.py audits the
    forked step (two steps, the static inputs overwritten in between).  The point, mesh and pyramid forks are there as ever; the mask
    fork is not taken -- the dual kernel reads the mask -- so the mask, the dual launch and the filter follow one another on the
    launch stream."""
    import stream_audit as sa
    import test_gpu_stream_audit as tsa
    from geometric_aware_dense_matching_amd import settings
    model = tsa._ffb6d()
    keys = ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")
    static, other = tsa._crops(131, keys), tsa._crops(132, keys)
    saved = (settings.USE_SIDE_STREAMS, list(settings.SIDE_PARTS), settings.MESH_FORK_LATE)
    pool, launch = ops.BufferPool(), tsa._launch_stream()

    def step(d):
        return infer.pipeline_step(model, d, **DUAL_KW)

    try:
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS, settings.MESH_FORK_LATE = True, ["mesh", "point", "pyr"], True
        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.stream(launch), ops.buffer_pool(pool):
            step(static)
            torch.cuda.synchronize()
            with sa.audited(known=sa.collect_tensors(model, pool, static, other)) as tr:
                step(static)
                for k, buf in static.items():
                    buf.copy_(other[k], non_blocking=True)
                forked = {k: v.clone() for k, v in step(static).items()}
        torch.cuda.synchronize()
    finally:
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS, settings.MESH_FORK_LATE = saved
    rep = sa.analyse(tr.log, unresolved=tr.unresolved)
    assert not rep.unresolved, rep.unresolved[:5]
    assert not rep.violations, "\n" + str(rep)
    assert rep.streams == {"main", "side0", "side1", "side2"}
    names = [(e.name, e.stream) for e in tr.log if e.kind == "access"]
    chain = ("gdm_seg_mask_hip", "gdm_match_dual_packed_hip", "gdm_match_score_hip", "gdm_match_cycle_hip")
    for entry in chain:
        assert names.count((entry, "main")) == 2 and sum(1 for n, _ in names if n == entry) == 2, entry
    assert [n for n, _ in names if n in chain] == list(chain) * 2
    with torch.no_grad():
        single = infer.pipeline_step(model, static, **DUAL_KW)
    ok, bad = infer.outputs_equal(single, forked)
    assert ok and set(single) == set(forked), bad
