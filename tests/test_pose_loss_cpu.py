"""CPU: the pose-fit loss (include/gdm.h THE POSE LOSS RULE) without a GPU -- the plain-torch reference against numpy and
gradcheck, the shared fit fragment and adjoint header in a g++ host build against fp64 autograd of that reference (and once more under
the address and undefined-behaviour sanitizers, as a stand-alone program), the loss module and its wiring on the reference path, the
entries' refusals and the command-line flags."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pose_loss_cases as pc
from geometric_aware_dense_matching_amd import loss, pose

SEEDS = (11, 12, 13)


@pytest.fixture(scope="module")
def cases():
    out = []
    for fam in pc.FAMILIES:
        for i, seed in enumerate(SEEDS):
            S = (1, 2, 6)[i]
            out.append(pc.make_case(fam, seed, S=S, winner=S - 1))
    return out


@pytest.fixture(scope="module")
def refs(cases):
    return [pc.reference(c) for c in cases]                        # computed once, shared, never modified


@pytest.fixture(scope="module")
def host(tmp_path_factory, cases):
    exe = pc.build_host(tmp_path_factory.mktemp("pose_adjoint"))
    raw, res = pc.run_host(exe, cases)
    return raw, res


def test_reference_forward_equals_numpy(cases, refs):
    """(1) fp64: the reference's pose is pose.kabsch_weighted_numpy's and its loss the numpy mean distance under the winning transform."""
    seen = 0
    for c, r in zip(cases, refs):
        if r["state"] != 0:
            continue
        RT = pose.kabsch_weighted_numpy(c["A"], c["B"], c["w"])
        assert np.abs(RT - r["RT"].astype(np.float64)).max() <= 1e-6          # the reference returns RT as f32
        D = []
        for s in range(len(c["sym"])):
            want = (c["X"] @ c["sym"][s, :, :3].T + c["sym"][s, :, 3]) @ c["gt"][:, :3].T + c["gt"][:, 3]
            D.append(np.linalg.norm(c["X"] @ RT[:, :3].T + RT[:, 3] - want, axis=1).mean())
        assert r["sym_idx"] == int(np.argmin(D)) == c["winner"]
        assert np.sort(D)[1] - np.min(D) > 1e-6 if len(D) > 1 else True
        assert abs(r["loss"] - min(D)) <= 1e-13
        seen += 1
    assert seen == len(pc.WELL) * len(SEEDS)


def test_reference_skip_rule_and_states():
    """Masked points and weights that are NaN, infinite, zero or negative are skipped exactly: the result equals that of the case
    without them; too few usable points is state 1 with the sentinel pose; a ground truth that is not finite is state 1."""
    c = pc.make_case("generic", 21, n=20)
    base = pc.reference(c)
    d = dict(c)
    rs = np.random.RandomState(0)
    d["A"] = np.concatenate([c["A"], rs.randn(5, 3)])
    d["B"] = np.concatenate([c["B"], rs.randn(5, 3)])
    d["w"] = np.concatenate([c["w"], [0.0, -1.0, np.nan, np.inf, 0.7]])
    mask = torch.ones(1, 25, dtype=torch.uint8)
    mask[0, 24] = 0
    got = pc.reference(d, mask=mask)
    assert got["state"] == 0 and got["loss"] == base["loss"]
    assert np.array_equal(got["dA"][:20], base["dA"]) and np.array_equal(got["dw"][:20], base["dw"])
    assert not got["dA"][20:].any() and not got["dw"][20:].any()
    few = pc.reference(pc.make_case("few", 3))
    assert few["state"] == 1 and few["loss"] == 0 and np.array_equal(few["RT"], pose.SENTINEL_RT.astype(np.float32))
    bad = dict(c)
    bad["gt"] = c["gt"].copy()
    bad["gt"][1, 3] = np.inf
    assert pc.reference(bad)["state"] == 1


def test_reference_gradcheck():
    """(2) torch.autograd.gradcheck of the reference in fp64 at n = 12, in the targets and the weights, with two symmetry transforms."""
    c = pc.make_case("generic", 5, n=12, K=8, S=2, winner=1)
    fixed = [torch.tensor(c[k], dtype=torch.float64) for k in ("B", "gt", "X", "sym")]

    def f(A, w):
        out = pose.kabsch_pose_loss_reference(fixed[0][None], A, w, fixed[1][None], fixed[2], fixed[3])
        assert int(out[2][0]) == 0
        return out[0]
    A = torch.tensor(c["A"], dtype=torch.float64)[None].requires_grad_(True)
    w = torch.tensor(c["w"], dtype=torch.float64)[None].requires_grad_(True)
    assert torch.autograd.gradcheck(f, (A, w), eps=1e-7, atol=1e-7, rtol=1e-5)


def test_reference_refuses_other_gradients():
    c = pc.make_case("generic", 5, n=12, K=8)
    t = {k: torch.tensor(c[k], dtype=torch.float64) for k in ("A", "B", "w", "gt", "X")}
    for name in ("B", "gt", "X"):
        args = dict(t)
        args[name] = t[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="not offered"):
            pose.kabsch_pose_loss_reference(args["B"][None], args["A"][None], args["w"][None], args["gt"][None], args["X"])


def test_adjoint_fragment_against_fp64_autograd(cases, refs, host):
    """(3) The g++ build of gdm_kabsch_fit.inc + gdm_pose_adjoint.h against fp64 autograd through torch.linalg.svd, per crop
    |got - ref| <= 1e-9 max|ref| over the crop's gradient (everything is fp64 and the gate caps the amplification at 1 / cond_min);
    state and winning transform equal; the gate leaves out none of the well-conditioned families; collinear points come back state 2
    and fewer than min_points state 1, with zero gradients."""
    _, res = host
    gated = 0
    for c, r, h in zip(cases, refs, res):
        tag = (c["family"], c["seed"])
        assert h["state"] == r["state"], tag
        assert h["sym_idx"] == r["sym_idx"], tag
        if c["family"] in pc.WELL:
            gated += r["state"] != 0
            if r["state"] != 0:
                continue
            assert abs(h["loss"] - r["loss"]) <= 1e-12 * max(1.0, r["loss"]), tag
            for k in ("dA", "dw"):
                ref = r[k]
                assert np.abs(ref).max() > 0, tag
                err = np.abs(h[k] - ref).max()
                print("%s seed %d %s: err %.3g of max %.3g" % (tag + (k, err, np.abs(ref).max())))
                assert err <= 1e-9 * np.abs(ref).max(), (tag, k, err, np.abs(ref).max())
        else:
            assert h["state"] == (2 if c["family"] == "collinear" else 1), tag
            assert h["loss"] == 0 and h["sym_idx"] == -1 and not h["dA"].any() and not h["dw"].any(), tag
    assert gated == 0


def test_adjoint_host_program_runs_clean_under_sanitizers(tmp_path, cases, host):
    """(4) The same host program under -fsanitize=address,undefined, a stand-alone binary: no report, and the same bits."""
    exe = pc.build_host(tmp_path, sanitize=True)
    raw, _ = pc.run_host(exe, cases)
    assert raw == host[0]


# ---- the loss module and its wiring, reference path -----------------------------------------------------------------------------------
def _batch(families=("generic", "collinear", "noisy", "few"), n=24, K=16):
    """A batch [B,n] from one case per family ("few": all but 4 weights zero)."""
    cs = [pc.make_case(f if f != "few" else "generic", 40 + i, n=n, K=K) for i, f in enumerate(families)]
    w = np.stack([c["w"] for c in cs])
    for i, f in enumerate(families):
        if f == "few":
            w[i, 4:] = 0
    t = lambda k: torch.tensor(np.stack([c[k] for c in cs]), dtype=torch.float64)
    return t("B"), t("A"), torch.tensor(w, dtype=torch.float64), t("gt"), torch.tensor(cs[0]["X"], dtype=torch.float64)


def test_pose_fit_loss_averages_the_fitted_crops():
    """(5) PoseFitLoss(match="reference") on the CPU: the mean over the state-0 crops only; a crop that is not fitted has no gradient."""
    scene, A, w, gt, X = _batch()
    fn = loss.PoseFitLoss(points=16, match="reference")
    A = A.requires_grad_(True)
    per, _, state, sym_idx = fn.per_crop(scene, A, w, gt, X)
    assert state.tolist() == [0, 2, 0, 1] and sym_idx.tolist() == [0, -1, 0, -1]
    value = fn(scene, A, w, gt, X)
    assert float(value) == float((per[0] + per[2]) / 2) and float(per[1]) == 0 and float(per[3]) == 0
    value.backward()
    assert A.grad[0].abs().max() > 0 and not A.grad[1].any() and not A.grad[3].any()
    none = fn(scene[1:2], A[1:2].detach(), w[1:2], gt[1:2], X)                  # no fitted crop: clamp(min=1), the value is 0
    assert float(none) == 0
    assert float(loss.PoseFitLoss(points=4, match="reference")(scene, A.detach(), w, gt, X)) != float(value)      # `points` selects X[:K]
    for bad in (dict(weights="conf"), dict(match="eager"), dict(points=0)):
        with pytest.raises(ValueError):
            loss.PoseFitLoss(**bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # the kernel path is never a fall-back either way
        loss.PoseFitLoss(points=16)(scene.float(), A.detach().float(), w.float(), gt.float(), X.float())


def _wiring_inputs(B=3, N=40, M=30, seed=8):
    rs = np.random.RandomState(seed)
    labels = (rs.rand(B, N) < 0.7).astype(np.int64)
    labels[1] = 0
    labels[1, :2] = 1                                            # 2 selected points: the item is skipped
    match = rs.randint(0, M, size=(B, N)).astype(np.int64)
    match[0, np.nonzero(labels[0])[0][:3]] = M                   # selected rows without a vertex: weight 0
    xyz = rs.uniform(-0.1, 0.1, (M, 3))
    q = np.stack([pc.rot(rs) for _ in range(B)])
    tr = rs.uniform(-0.2, 0.2, (B, 3)) + [0, 0, 0.8]
    cld = np.zeros((B, 9, N))
    cld[:, :3] = np.einsum("bij,bnj->bin", q, xyz[match.clip(0, M - 1)]) + tr[:, :, None] + 1e-3 * rs.randn(B, 3, N)
    gt = np.concatenate([np.einsum("ij,bjk->bik", pc.rot(rs, 0.03), q), tr[:, :, None] + 0.005], axis=2)
    m = rs.randn(16, M)
    f = np.zeros((B, 16, N))
    f[:] = m[:, match.clip(0, M - 1)].transpose(1, 0, 2) + 0.3 * rs.randn(B, 16, N)      # descriptors near their vertex: sharp assignments
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return tt(labels), tt(match), tt(f), tt(m), tt(xyz), tt(gt), tt(cld)


def _terms(model, f, m, xyz, labels, match, x, static, sym_idx=None):
    """The selection of pointwise_feature_matching (compacted or static all-rows form), then loss.soft_assign_terms in fp64."""
    B, D, N = f.shape
    sel = labels == 1
    counts = sel.sum(1)
    sel = sel & (counts >= 3).unsqueeze(1)
    if static:
        bi, pi = torch.arange(B).repeat_interleave(N), torch.arange(N).repeat(B)
    else:
        bi, pi = torch.nonzero(sel, as_tuple=True)
    rows = torch.nn.functional.normalize(f.transpose(1, 2)[bi, pi], dim=1)
    mesh_rows = torch.nn.functional.normalize(m, dim=0).t().contiguous()
    c1 = match[bi, pi]
    c2 = match[bi, sym_idx[pi]] if sym_idx is not None else None
    return loss.soft_assign_terms(model, rows, mesh_rows, xyz, c1, c2, bi, pi, counts, x, static_shape=(B, N) if static else None,
                                  row_weight=sel.reshape(-1) if static else None)


def _model(**kw):
    base = dict(soft_gamma=16.0, soft_beta=0.005, soft_xyz_weight=0.0, soft_nll_weight=1.0, soft_match="reference")
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("weights", ["uniform", "prob"])
def test_wiring_static_and_compacted_forms_agree_with_a_direct_call(weights):
    """(5) soft_assign_terms with pose_loss_weight set: the third value, in the compacted (scatter) and the static all-rows form, equals
    PoseFitLoss on the soft vertices and row weights formed here by hand; "prob" weights are exp(-nll) of the likelihood term's rows."""
    labels, match, f, m, xyz, gt, cld = _wiring_inputs()
    B, _, N = f.shape
    M = m.shape[1]
    x = dict(RT=gt, cld_rgb_nrm=cld)
    model = _model(pose_loss_weight=0.5, pose_loss_points=20, pose_loss_weights=weights)
    vals, grads = [], []
    for static in (False, True):
        ff = f.clone().requires_grad_(True)
        lx, ln, lp = _terms(model, ff, m, xyz, labels, match, x, static)
        assert float(lx) == 0.0 and float(ln) > 0 and float(lp) > 0
        lp.backward()
        vals.append(float(lp))
        grads.append(ff.grad.clone())
    assert abs(vals[0] - vals[1]) <= 1e-15 and (grads[0] - grads[1]).abs().max().item() <= 1e-15
    rows = torch.nn.functional.normalize(f.transpose(1, 2).reshape(B * N, -1), dim=1)
    mesh_rows = torch.nn.functional.normalize(m, dim=0).t()
    lse, soft = loss.soft_coord_reference(rows, mesh_rows, xyz, 16.0)
    sel = (labels == 1) & ((labels == 1).sum(1) >= 3).unsqueeze(1)
    w = (sel & (match < M)).to(torch.float64).reshape(-1)
    if weights == "prob":
        nll = lse - 16.0 * (rows * mesh_rows[match.reshape(-1).clamp(0, M - 1)]).sum(1)
        w = w * torch.exp(-nll)
    direct = loss.PoseFitLoss(points=20, weights=weights, match="reference")(cld, soft.view(B, N, 3), w.view(B, N), gt, xyz)
    assert abs(float(direct) - vals[0]) <= 1e-15
    assert not grads[0][1].any()                                 # the skipped item gets no gradient


def test_wiring_refusals():
    """(5) Symmetric models and a batch without RT are refused; so is the term inside SoftAssignLoss for symmetric rows."""
    labels, match, f, m, xyz, gt, cld = _wiring_inputs(N=30, M=30)
    model = _model(pose_loss_weight=1.0)
    with pytest.raises(ValueError, match="RT"):
        _terms(model, f, m, xyz, labels, match, dict(cld_rgb_nrm=cld), False)
    with pytest.raises(ValueError, match="symmetric"):
        _terms(model, f, m, xyz, labels, match, dict(RT=gt, cld_rgb_nrm=cld), False, sym_idx=torch.from_numpy(np.random.RandomState(7).permutation(30)))


@pytest.mark.parametrize("static", [False, True])
def test_weight_zero_leaves_the_step_bit_for_bit(static):
    """(5) pose_loss_weight = 0 against the attribute absent: the same two values and the same gradients of a tiny reference-path step,
    bit for bit, and still a pair -- the term does not exist when it is off."""
    labels, match, f0, m0, xyz, gt, cld = _wiring_inputs()
    x = dict(RT=gt, cld_rgb_nrm=cld)
    res = []
    for model in (_model(soft_xyz_weight=1.0), _model(soft_xyz_weight=1.0, pose_loss_weight=0.0, pose_loss_points=20, pose_loss_weights="prob")):
        f, m = f0.clone().requires_grad_(True), m0.clone().requires_grad_(True)
        out = _terms(model, f, m, xyz, labels, match, x, static)
        assert len(out) == 2
        (out[0] + 0.01 * out[1]).backward()
        res.append((out[0].detach(), out[1].detach(), f.grad, m.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_models_carry_the_attributes_and_flags_parse():
    from geometric_aware_dense_matching_amd import train_lm
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    for cls in (GeoMatch, GeoMatchDGCNN):
        assert (cls.pose_loss_weight, cls.pose_loss_points, cls.pose_loss_weights) == (0.0, 256, "uniform")
    a = train_lm.build_parser().parse_args([])
    assert (a.pose_loss_weight, a.pose_loss_points, a.pose_loss_weights) == (0.0, 256, "uniform")
    off = SimpleNamespace()
    train_lm._set_soft_losses(off, a)
    assert not vars(off)                                         # off: the class defaults stay untouched
    a = train_lm.build_parser().parse_args(["--pose-loss-weight", "0.5", "--pose-loss-points", "128", "--pose-loss-weights", "prob",
                                            "--soft-gamma", "8"])
    on = SimpleNamespace()
    train_lm._set_soft_losses(on, a)
    assert vars(on) == dict(soft_gamma=8.0, pose_loss_weight=0.5, pose_loss_points=128, pose_loss_weights="prob")
    with pytest.raises(SystemExit):
        train_lm.build_parser().parse_args(["--pose-loss-weights", "conf"])


def test_entries_refuse_before_any_device_call():
    """NULL, B / N / K / S < 1, S above the cap, bad strides, a short or misaligned record, a cond_min outside [0, 1): GDM_EINVAL with
    a message before any HIP call (host pointers, no GPU)."""
    from geometric_aware_dense_matching_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    nb = lib.gdm_pose_loss_record_bytes(4)
    assert nb == 4 * 48 * 8 + 16 and lib.gdm_pose_loss_record_bytes(0) == 0 and lib.gdm_pose_loss_record_bytes(3) == 3 * 48 * 8 + 16
    cap = pose.POSE_LOSS["GDM_POSE_LOSS_MAX_S"]
    assert cap == 64 and pose.POSE_LOSS["GDM_POSE_LOSS_REC"] == 32

    def fwd(scene=p, sb=24, ps=3, cs=1, B=4, N=8, K=8, S=1, cond=1e-3, rec=p, rbytes=nb, sym=p):
        return lib.gdm_pose_loss_fwd_hip(scene, sb, ps, cs, p, p, p, p, p, sym, B, N, K, S, 5, cond, rec, rbytes, p, p, p, p, None)

    def bwd(sb=24, ps=3, cs=1, B=4, N=8, rec=p, rbytes=nb, grad=p):
        return lib.gdm_pose_loss_bwd_hip(p, sb, ps, cs, p, p, p, rec, rbytes, grad, B, N, p, p, None)
    for kw, word in ((dict(scene=None), b"NULL"), (dict(B=0), b"bad shape"), (dict(N=0), b"bad shape"), (dict(K=0), b"bad shape"),
                     (dict(S=0), b"S=0"), (dict(S=cap + 1), b"S=65"), (dict(S=2, sym=None), b"symmetry"), (dict(ps=0), b"strides"),
                     (dict(cs=0), b"strides"), (dict(sb=-1), b"strides"), (dict(B=70000), b"65535"), (dict(rbytes=nb - 1), b"record"),
                     (dict(rec=p + 4), b"record"), (dict(cond=1.0), b"cond_min"), (dict(cond=-0.1), b"cond_min"),
                     (dict(cond=float("nan")), b"cond_min")):
        assert fwd(**kw) == -1, kw
        assert word in lib.gdm_last_error(), (kw, lib.gdm_last_error())
    for kw, word in ((dict(grad=None), b"NULL"), (dict(B=0), b"bad shape"), (dict(N=-1), b"bad shape"), (dict(ps=0), b"strides"),
                     (dict(rbytes=0), b"record"), (dict(rec=p + 4), b"record")):
        assert bwd(**kw) == -1, kw
        assert word in lib.gdm_last_error(), (kw, lib.gdm_last_error())
