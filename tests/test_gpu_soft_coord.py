"""GPU: ops.soft_coord_match (csrc/gdm_softcoord.hip) and loss.SoftAssignLoss against fp64 -- forward and backward within the derived
bounds of DESIGN.md 6l (soft_coord_cases.bounds), no [R, M] array, bit-identical runs, weightless padding, the loss wired into both
model variants (value, gradients, static all-rows form, defaults untouched) and the captured training step with the losses on."""
import functools
import math

import numpy as np
import pytest
import torch

import soft_coord_cases as sc
from geometric_aware_dense_matching_amd import loss, ops, settings, synthetic
from geometric_aware_dense_matching_amd.config import make_dgcnn_cfg, make_model_cfg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 31), (127, 64), (128, 65), (129, 130), (300, 1000), (257, 4097)]
GAMMAS = [1.0, 16.0, 40.0]
U = sc.U


@functools.lru_cache(maxsize=None)
def _reference(R, M, gamma, family):
    """Inputs and the fp64 reference of one case, computed once and shared by the forward and backward tests (never modified)."""
    x, y, xyz, a, b = sc.make_case(R, M, seed=1000 * R + M, family=family)
    t64 = [torch.from_numpy(v).double() for v in (x, y, xyz, a, b)]
    ref = sc.analytic(*t64, gamma)
    lse, soft = loss.soft_coord_reference(t64[0], t64[1], t64[2], gamma)
    assert (lse - ref["lse"]).abs().max() <= 1e-12 and (soft - ref["soft"]).abs().max() <= 1e-12
    return (x, y, xyz, a, b), ref, sc.bounds(ref, t64[4], t64[2], gamma, R, M)


def _run(x, y, xyz, a, b, gamma):
    xd, yd = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y).cuda().requires_grad_(True)
    lse, soft = ops.soft_coord_match(xd, yd, torch.from_numpy(xyz).cuda(), gamma)
    ((lse * torch.from_numpy(a).cuda()).sum() + (soft * torch.from_numpy(b).cuda()).sum()).backward()
    return lse.detach(), soft.detach(), xd.grad, yd.grad


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("R, M", SHAPES)
def test_forward_within_the_bounds_of_6k(R, M, gamma):
    """(1) |lse - lse64| <= gamma delta + 1e-5 and |soft - soft64|inf <= E rho + 1e-6, random unit rows and the bit-copy family."""
    for family in ("random", "copy"):
        (x, y, xyz, a, b), ref, bnd = _reference(R, M, gamma, family)
        lse, soft = ops.soft_coord_match(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(xyz).cuda(), gamma)
        e_lse = (lse.double().cpu() - ref["lse"]).abs().max().item()
        e_soft = (soft.double().cpu() - ref["soft"]).abs().max().item()
        print("fwd %-6s R=%d M=%d gamma=%g: |lse err| %.3e (bound %.3e)  |soft err| %.3e (bound %.3e)"
              % (family, R, M, gamma, e_lse, bnd["lse"], e_soft, bnd["soft"]))
        assert lse.shape == (R,) and soft.shape == (R, 3)
        assert e_lse <= bnd["lse"] and e_soft <= bnd["soft"]


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("R, M", SHAPES)
def test_backward_within_the_derived_bounds(R, M, gamma):
    """(2) per component: |gx_r - gx64_r| <= (E + 2^-14 + (M+128) u) A_r + 2 gamma E rho |b_r|_1 + 1e-7 and the same for gy with
    (R+128) u, A'_c and sum_r p_rc |b_r|_1; and the scale-free max|got - want| / max|want| < 1e-2 on each gradient."""
    for family in ("random", "copy"):
        (x, y, xyz, a, b), ref, bnd = _reference(R, M, gamma, family)
        _, _, gx, gy = _run(x, y, xyz, a, b, gamma)
        ex = (gx.double().cpu() - ref["gx"]).abs().numpy()
        ey = (gy.double().cpu() - ref["gy"]).abs().numpy()
        rx, ry = ex.max() / ref["gx"].abs().max().item(), ey.max() / ref["gy"].abs().max().item()
        print("bwd %-6s R=%d M=%d gamma=%g: gx err/bound %.3e rel %.3e   gy err/bound %.3e rel %.3e"
              % (family, R, M, gamma, (ex.max(1) / bnd["gx"]).max(), rx, (ey.max(1) / bnd["gy"]).max(), ry))
        assert gx.shape == (R, 128) and gy.shape == (M, 128)
        assert (ex <= bnd["gx"][:, None]).all() and (ey <= bnd["gy"][:, None]).all()
        assert rx < 1e-2 and ry < 1e-2


def test_no_r_by_m_array():
    """(3) R = 32768, M = 4096: the growth of max_memory_allocated over the inputs across forward + backward stays below 256 MiB,
    half of one f32 [R, M]."""
    R, M = 32768, 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(R, 128, device="cuda", generator=g), dim=1).requires_grad_(True)
    y = torch.nn.functional.normalize(torch.randn(M, 128, device="cuda", generator=g), dim=1).requires_grad_(True)
    xyz = torch.rand(M, 3, device="cuda", generator=g) * 0.2 - 0.1
    a, b = torch.randn(R, device="cuda", generator=g), torch.randn(R, 3, device="cuda", generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lse, soft = ops.soft_coord_match(x, y, xyz, 16.0)
    ((lse * a).sum() + (soft * b).sum()).backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print("peak growth %.1f MiB" % (grown / 2 ** 20))
    assert grown < 256 * 2 ** 20
    assert torch.isfinite(lse).all() and torch.isfinite(x.grad).all() and torch.isfinite(y.grad).all()
    assert (soft.abs() <= 0.1 + 1e-6).all()                        # a convex combination of the vertices


def test_bit_identical_runs_and_weightless_padding():
    """(4) two forward + backward runs are bit-identical; at (R, M) = (129, 130): 127 zero rows appended to x with zero upstream
    gradients change nothing on the real rows and add exactly nothing to gy; the entry points called with the operands of a
    256-row zero-padded y, an xyz buffer and per-row buffers that hold NaN beyond M and R give the same bits (nothing beyond M or R
    is read into a result); gamma = 0, 40.5 and NaN are refused with no launch."""
    from geometric_aware_dense_matching_amd import _lib
    R, M, gamma = 129, 130, 16.0
    (x, y, xyz, a, b), _, _ = _reference(R, M, gamma, "copy")
    first, again = _run(x, y, xyz, a, b, gamma), _run(x, y, xyz, a, b, gamma)
    for p, q in zip(first, again):
        assert torch.equal(p, q)
    lse, soft, gx, gy = first
    pad = lambda v, n: np.concatenate([v, np.zeros((n - v.shape[0],) + v.shape[1:], v.dtype)])
    lse2, soft2, gx2, gy2 = _run(pad(x, 256), y, xyz, pad(a, 256), pad(b, 256), gamma)
    assert torch.equal(lse2[:R], lse) and torch.equal(soft2[:R], soft) and torch.equal(gx2[:R], gx) and torch.equal(gy2, gy)
    assert gx2[R:].abs().max().item() == 0
    # the C entries with poisoned padding
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    xr, xt, _ = ops._cm_pack(torch.from_numpy(x).cuda())
    yr, yt, _ = ops._cm_pack(torch.from_numpy(pad(y, 256)).cuda())
    nan = float("nan")
    xyzp = torch.full((256, 3), nan, device="cuda")
    xyzp[:M] = torch.from_numpy(xyz).cuda()
    lse3, soft3 = torch.full((256,), nan, device="cuda"), torch.full((256, 3), nan, device="cuda")
    assert L.gdm_soft_coord_fwd_hip(xr.data_ptr(), xt.data_ptr(), yr.data_ptr(), yt.data_ptr(), xyzp.data_ptr(), R, M, gamma,
                                    lse3.data_ptr(), soft3.data_ptr(), st) == 0
    assert torch.equal(lse3[:R], lse) and torch.equal(soft3[:R], soft)
    assert torch.isnan(lse3[R:]).all() and torch.isnan(soft3[R:]).all()          # nothing is written beyond R either
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    kb = torch.full((256, 4), nan, device="cuda")
    kb[:R] = torch.cat([(ad - (bd * soft).sum(1)).unsqueeze(1), bd], dim=1)
    P = L.gdm_soft_coord_bwd_parts(R, M)
    gx3, gy3 = torch.full((256, 128), nan, device="cuda"), torch.empty((M, 128), device="cuda")
    part = torch.empty((P, 256, 128), device="cuda")
    assert L.gdm_soft_coord_bwd_hip(xr.data_ptr(), xt.data_ptr(), yr.data_ptr(), yt.data_ptr(), xyzp.data_ptr(), R, M, gamma, lse3.data_ptr(),
                                    kb.data_ptr(), gx3.data_ptr(), part.data_ptr(), gy3.data_ptr(), st) == 0
    assert torch.equal(gx3[:R], gx) and torch.equal(gy3, gy) and torch.isnan(gx3[R:]).all()
    assert part[:, M:].abs().max().item() == 0                    # a padded vertex gets no gradient
    # refused before any launch
    xd, yd, zd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(xyz).cuda()
    for bad in (0.0, 40.5, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            ops.soft_coord_match(xd, yd, zd, bad)
        assert L.gdm_soft_coord_fwd_hip(xr.data_ptr(), xt.data_ptr(), yr.data_ptr(), yt.data_ptr(), xyzp.data_ptr(), R, M, bad,
                                        lse3.data_ptr(), soft3.data_ptr(), st) == -1


# ---- loss level ------------------------------------------------------------------------------------------------------------------------
def _model(M, N, seed=0):
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    torch.manual_seed(seed)
    m = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M)).cuda().train()
    m.model_emb.dropout = 0.0
    return m


def _loss_batch(B, N, M, with_rt, seed=1):
    rs = np.random.RandomState(seed)
    labels = (rs.rand(B, N) < 0.5).astype(np.int32)
    labels[1] = 0
    labels[1, :2] = 1                                            # 2 selected points: the item is skipped
    match = rs.randint(0, M + 1, size=(B, N)).astype(np.int32)
    x = dict(labels=torch.from_numpy(labels).cuda(), match_idx=torch.from_numpy(match).cuda(),
             visible_flag=torch.from_numpy((rs.rand(B, M) < 0.6).astype(np.float32)).cuda())
    if with_rt:
        q = np.stack([np.linalg.qr(rs.randn(3, 3))[0] for _ in range(B)])
        x["RT"] = torch.from_numpy(np.concatenate([q, rs.randn(B, 3, 1) * 0.3], axis=2).astype(np.float32)).cuda()
        x["cld_rgb_nrm"] = torch.from_numpy((rs.randn(B, 9, N) * 0.1).astype(np.float32)).cuda()
    f0 = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32)).cuda()
    m0 = torch.from_numpy(rs.randn(1, 128, M).astype(np.float32)).cuda()
    return x, f0, m0


def _pfm(model, f0, m0, x, weights):
    model.soft_xyz_weight, model.soft_nll_weight = weights
    f, m = f0.clone().requires_grad_(True), m0.clone().requires_grad_(True)
    v = model.pointwise_feature_matching(f, m, x)
    v.backward()
    return v.detach().double().cpu(), f.grad.double().cpu(), m.grad.double().cpu()


def _loss_tolerances(f64, m64, xyz64, labels, match, gamma, beta, RT, cld):
    """Bounds on (value, d/df, d/dm) of the two soft losses (weights 1) of the fp32 path against fp64, from the operator's bounds
    (soft_coord_cases.bounds) scaled by the row weights omega_r = 1 / (rows of the item x items):
      * the operator's gx / gy bounds with upstream a_r = omega_r, b_r = omega_r smooth_l1'(soft_r - t_r);
      * b_r itself is formed from the kernel's soft_r, off by at most E rho + 1e-6, and smooth_l1' has slope 1 / beta:
        |db_r|_1 <= 3 omega_r min(2, (E rho + 1e-6) / beta), which moves G_rc by at most gamma p_rc |db_r|_1 2 rho;
      * the ground-truth column's term gamma <x_r, y_g> and its gradients are fp32 torch: 8 u gamma omega_r per row;
      * through F.normalize: |J e|_inf <= |e|_2 / |f| <= sqrt(128) |e|_inf / |f|.
    Value: sum_r omega_r (gamma delta + 1e-5 + 8 u gamma + 3 (E rho + 1e-6)) (smooth_l1 is 1-Lipschitz)."""
    B, D, N = f64.shape
    M = m64.shape[1]
    sel = labels == 1
    counts = sel.sum(1)
    ok = counts >= 3
    sel = sel & ok[:, None]
    bi, pi = torch.nonzero(sel, as_tuple=True)
    g = match[bi, pi]
    omega = (1.0 / (counts[bi].double() * ok.sum())) * (g < M)
    rows, y = f64.transpose(1, 2)[bi, pi], m64.t()
    x = rows / rows.norm(dim=1, keepdim=True)
    yn = y / y.norm(dim=1, keepdim=True)
    lse, soft = loss.soft_coord_reference(x, yn, xyz64, gamma)
    gc = g.clamp(max=M - 1)
    t = xyz64[gc] if RT is None else torch.einsum("rj,rjk->rk", cld.transpose(1, 2)[bi, pi] - RT[bi, :, 3], RT[bi, :, :3])
    d = soft - t
    b = omega[:, None] * torch.where(d.abs() < beta, d / beta, torch.sign(d))
    ref = sc.analytic(x, yn, xyz64, omega, b, gamma)
    bnd = sc.bounds(ref, b, xyz64, gamma, x.shape[0], M)
    E, rho = bnd["E"], bnd["rho"]
    db1 = 3 * omega * min(2.0, (E * rho + 1e-6) / beta)
    ex = torch.from_numpy(bnd["gx"]) + gamma * 2 * rho * db1 + 8 * U * gamma * omega
    per_col = torch.zeros(M, dtype=torch.float64).index_add_(0, gc, omega)
    ey = torch.from_numpy(bnd["gy"]) + gamma * 2 * rho * (ref["p"] * db1[:, None]).sum(0) + (x.shape[0] + 8) * U * gamma * per_col
    tol_f = torch.zeros(B, N, dtype=torch.float64)
    tol_f[bi, pi] = math.sqrt(128) * ex / rows.norm(dim=1)
    tol_m = math.sqrt(128) * ey / y.norm(dim=1)
    tol_v = (omega * (gamma * sc.DELTA + 1e-5 + 8 * U * gamma + 3 * (E * rho + 1e-6))).sum().item()
    return tol_v, tol_f, tol_m


@pytest.mark.parametrize("target", ["RT", "vertex"])
def test_loss_value_and_gradients_equal_the_fp64_loop(target):
    """(5) B = 3, N = M = 512, one item of 2 selected points: pointwise_feature_matching with both weights 1 minus the same with both
    weights 0 (value, d/d features, d/d mesh) against soft_coord_cases.loop_loss in fp64 on the same tensors, within
    _loss_tolerances plus the fp32 rounding of the sums that cancel (16 u of the circle loss, 4 u of its gradients)."""
    B, N, M = 3, 512, 512
    model = _model(M, N)
    x, f0, m0 = _loss_batch(B, N, M, with_rt=target == "RT")
    v1, gf1, gm1 = _pfm(model, f0, m0, x, (1.0, 1.0))
    v0, gf0, gm0 = _pfm(model, f0, m0, x, (0.0, 0.0))
    f64, m64 = f0.double().cpu().requires_grad_(True), m0[0].double().cpu().requires_grad_(True)
    xyz64 = model.model_emb.xyz.double().cpu()
    labels, match = x["labels"].long().cpu(), x["match_idx"].long().cpu()
    RT = x["RT"].double().cpu() if target == "RT" else None
    cld = x["cld_rgb_nrm"][:, :3].double().cpu() if target == "RT" else None
    lx, ln = sc.loop_loss(f64, m64, xyz64, labels, match, model.soft_gamma, model.soft_beta, RT=RT, cld=cld)
    (lx + ln).backward()
    tol_v, tol_f, tol_m = _loss_tolerances(f64.detach(), m64.detach(), xyz64, labels, match, model.soft_gamma, model.soft_beta, RT, cld)
    dv = abs((v1 - v0).item() - (lx + ln).item())
    df = ((gf1 - gf0) - f64.grad).abs()
    dm = ((gm1 - gm0)[0] - m64.grad).abs()
    lim_f = tol_f[:, None, :] + 4 * U * gf1.abs() + 64 * U * f64.grad.abs().max()
    lim_m = tol_m[None, :] + 4 * U * gm1[0].abs() + 64 * U * m64.grad.abs().max()
    print("loss %s: soft value %.6f (xyz %.6f nll %.4f) err %.3e tol %.3e; d/df err/lim %.3e, d/dm err/lim %.3e; rel %.3e %.3e"
          % (target, (lx + ln).item(), lx.item(), ln.item(), dv, tol_v, (df / lim_f).max(), (dm / lim_m).max(),
             df.max() / f64.grad.abs().max(), dm.max() / m64.grad.abs().max()))
    assert lx.item() > 0 and ln.item() > 0
    assert dv <= tol_v + 16 * U * abs(v1.item())
    assert (df <= lim_f).all() and (dm <= lim_m).all()
    assert gf1[1].sub(gf0[1]).abs().max().item() == 0             # the skipped item gets nothing from the soft losses


def test_static_rows_form_equals_compacted_form():
    """(5) settings.STATIC_MATCH_ROWS with the losses on: value and both gradients equal the compacted form's, as
    tests/test_gpu_train_graph.py holds the circle loss alone."""
    B, N, M = 3, 512, 512
    model = _model(M, N)
    x, f0, m0 = _loss_batch(B, N, M, with_rt=True)
    res = []
    try:
        for static in (False, True):
            settings.STATIC_MATCH_ROWS = static
            res.append(_pfm(model, f0, m0, x, (1.0, 1.0)))
    finally:
        settings.STATIC_MATCH_ROWS = False
    (l0, gf0, gm0), (l1, gf1, gm1) = res
    assert np.isfinite(l0.item()) and abs(l0 - l1).item() < 1e-6 * abs(l0.item())
    assert gf0[1].abs().max().item() == 0 and gf1[1].abs().max().item() == 0
    assert (gf1 - gf0).abs().max().item() < 1e-6 * gf0.abs().max().item() + 1e-9
    assert (gm1 - gm0).abs().max().item() < 2e-5 * gm0.abs().max().item()             # summation order over the rows differs


def test_defaults_never_call_the_operator(monkeypatch):
    """(5) both weights 0 and ops.soft_coord_match replaced by a function that raises: a training forward runs, and end_points has
    exactly today's keys; with a weight set the same forward reaches the operator."""
    from geometric_aware_dense_matching_amd import train_lm
    M, N, B = 512, 1024, 2                                        # N = 1024: the smallest cloud the neighbour pyramid accepts
    model = _model(M, N, seed=7)
    ds = train_lm.SyntheticCrops(B, N, M, seed=3)
    batch = torch.utils.data.default_collate([ds[i] for i in range(B)])

    def boom(*args, **kwargs):
        raise AssertionError("soft_coord_match called")

    monkeypatch.setattr(ops, "soft_coord_match", boom)
    assert (model.soft_xyz_weight, model.soft_nll_weight) == (0.0, 0.0)
    out, _ = train_lm.model_fn_dec(model, batch, torch.device("cuda", 0))
    assert sorted(out) == sorted(["loss", "seg_loss", "match_loss", "seg", "mesh", "rgbd"])
    model.soft_nll_weight = 0.5
    with pytest.raises(AssertionError, match="soft_coord_match called"):
        train_lm.model_fn_dec(model, batch, torch.device("cuda", 0))


def test_dgcnn_variant_adds_the_same_losses():
    """(5) the DGCNN variant's pointwise_feature_matching (selection by origin_labels, the mesh buffer's coordinates, RT target):
    weights 1 minus weights 0 against the fp64 loop, same tolerances."""
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    B, N, M = 3, 512, 512
    torch.manual_seed(0)
    model = GeoMatchDGCNN(make_dgcnn_cfg(n_mesh_node=M, dataset="ycbv"), 2, model_points=synthetic.make_model_points(2, M, 269.573)).cuda().train()
    x, f0, m0 = _loss_batch(B, N, M, with_rt=True, seed=2)
    x["origin_labels"] = x["labels"]
    x["RT"][:, 2, 3] = x["RT"][:, 2, 3].abs() + 0.6              # in front of the camera: the positive radius scales with depth
    v1, gf1, gm1 = _pfm(model, f0, m0, x, (1.0, 1.0))
    v0, gf0, gm0 = _pfm(model, f0, m0, x, (0.0, 0.0))
    f64, m64 = f0.double().cpu().requires_grad_(True), m0[0].double().cpu().requires_grad_(True)
    xyz64 = model.model_emb.mesh[0][:3].t().double().cpu()
    labels, match = x["labels"].long().cpu(), x["match_idx"].long().cpu()
    RT, cld = x["RT"].double().cpu(), x["cld_rgb_nrm"][:, :3].double().cpu()
    lx, ln = sc.loop_loss(f64, m64, xyz64, labels, match, model.soft_gamma, model.soft_beta, RT=RT, cld=cld)
    (lx + ln).backward()
    tol_v, tol_f, tol_m = _loss_tolerances(f64.detach(), m64.detach(), xyz64, labels, match, model.soft_gamma, model.soft_beta, RT, cld)
    dv = abs((v1 - v0).item() - (lx + ln).item())
    df = ((gf1 - gf0) - f64.grad).abs()
    dm = ((gm1 - gm0)[0] - m64.grad).abs()
    assert dv <= tol_v + 16 * U * abs(v1.item())
    assert (df <= tol_f[:, None, :] + 4 * U * gf1.abs() + 64 * U * f64.grad.abs().max()).all()
    assert (dm <= tol_m[None, :] + 4 * U * gm1[0].abs() + 64 * U * m64.grad.abs().max()).all()


def test_graphed_training_step_with_the_losses_on():
    """(6) B = 2, M = 512, N = 1024 (the smallest cloud the neighbour pyramid accepts), four iterations with soft_xyz_weight = soft_nll_weight = 1: GraphedTrainStep (3 eager warm-up
    iterations, one capture, one replay) against the eager loop, all five loss values held to 10x what the eager loop differs from
    itself run twice or 2e-4 relative, whichever is larger (test_graphed_training_iterations_equal_the_eager_loop's yardstick).
    The learning rate climbs from 1e-7 to 1e-6 (a cyclic schedule stepped on both sides, read from the device by the capture): Adam's
    update is sign-like, so every step turns the summation-order noise of the atomics into parameter differences of the size of the
    learning rate, which train-mode BatchNorm on two items amplifies chaotically; at 1e-5 two EAGER runs differ by 4e-2 in one
    iteration and 6e-4 in the next, and a single sample of that is no yardstick."""
    from geometric_aware_dense_matching_amd import train_lm
    from geometric_aware_dense_matching_amd.train_graph import GraphedTrainStep
    M, N, B, steps = 512, 1024, 2, 4
    dev = torch.device("cuda", 0)
    ds = train_lm.SyntheticCrops(B * steps, N, M, seed=3)
    batches = [torch.utils.data.default_collate([ds[s * B + i] for i in range(B)]) for s in range(steps)]
    keys = ("loss", "seg_loss", "match_loss", "soft_xyz_loss", "soft_nll_loss")

    def run(graphed):
        model = _model(M, N, seed=7)
        model.soft_xyz_weight = model.soft_nll_weight = 1.0
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        stepper = GraphedTrainStep(model, opt, dev) if graphed else None
        sched = torch.optim.lr_scheduler.CyclicLR(opt, base_lr=1e-7, max_lr=1e-6, cycle_momentum=False, step_size_up=4, step_size_down=4)
        losses = []
        for b in batches:
            if graphed:
                out = stepper.step(b)
            else:
                out, _ = train_lm.model_fn_dec(model, b, dev)
                out["loss"].backward()
                opt.step()
                opt.zero_grad()
            losses.append([float(torch.as_tensor(out[k]).detach()) for k in keys])
            sched.step()
        return np.array(losses), stepper

    le, _ = run(False)
    le2, _ = run(False)
    lg, stepper = run(True)
    assert stepper.captures == 1 and stepper.calls == steps
    noise = np.abs(le2 - le).max(axis=1)
    diff = np.abs(lg - le).max(axis=1)
    print("eager  ", le, "\ngraphed", lg, "\neager-vs-eager", noise, "\ngraph-vs-eager", diff)
    assert np.isfinite(lg).all() and (lg[:, 3:] > 0).all()
    assert (diff <= np.maximum(10.0 * noise, 2e-4 * np.abs(le).max(axis=1))).all(), (diff, noise)
