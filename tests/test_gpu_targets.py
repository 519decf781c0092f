"""GPU: ground-truth correspondence targets (csrc/gdm_targets.hip) -- the flip, the hidden-point removal and get_pose_gt_info
against golden vectors made by the real reference (tests/golden/make_golden_targets.py), with exact equality; batch independence,
shared vs per-crop models, permutation equivariance, eager / hipGraph bit-identity, and the front end's origin_labels."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from geometric_aware_dense_matching_amd import synthetic, targets  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
CASES = "abcdef"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "pose_targets.npz")))


def _case(g, c):
    RT = g[c + "_RT"]
    B = RT.shape[0]
    model = g[c + "_model"]
    M = model.shape[-2]
    bits = lambda k: np.unpackbits(g[c + "_" + k], axis=1)[:, :M]            # noqa: E731
    return dict(RT=RT, B=B, M=M, model=model, cld=g[c + "_cld"], labels=g[c + "_labels"], inv_t=g[c + "_inv_t"],
                vis_ref=bits("vis_ref"), vis_def=bits("vis_def"), labels_out=g[c + "_labels_out"],
                match_idx=g[c + "_match_idx"].astype(np.int32), visible_flag=bits("visible_flag"), valid=g[c + "_valid"])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("c", ["b", "e"])
def test_flipped_points_bit_equal_to_reference(gold, c):
    d = _case(gold, c)
    _, f = targets.visible_vertices(_t(d["model"]), _t(d["RT"]), cam_center=_t(d["inv_t"]), return_flipped=True)
    assert np.array_equal(f[0].cpu().numpy(), gold[c + "_flipped0"])


@pytest.mark.parametrize("c", CASES)
def test_flipped_points_equal_documented_formula(gold, c):
    d = _case(gold, c)
    _, f = targets.visible_vertices(_t(d["model"]), _t(d["RT"]), return_flipped=True)
    cam = targets.default_cam_center(d["RT"])
    for b in range(d["B"]):
        m = d["model"] if d["model"].ndim == 2 else d["model"][b]
        assert np.array_equal(f[b].cpu().numpy(), targets.spherical_flip(m, cam[b])), b


@pytest.mark.parametrize("c", CASES)
@pytest.mark.parametrize("centre", ["reference", "default"])
def test_visibility_equals_reference(gold, c, centre):
    d = _case(gold, c)
    cam = _t(d["inv_t"]) if centre == "reference" else None
    vis = targets.visible_vertices(_t(d["model"]), _t(d["RT"]), cam_center=cam).cpu().numpy()
    want = d["vis_ref"] if centre == "reference" else d["vis_def"]
    for b in range(d["B"]):
        assert np.array_equal(vis[b], want[b]), "crop %d: %d differ of %d" % (b, int((vis[b] != want[b]).sum()), int(want[b].sum()))


@pytest.mark.parametrize("c", CASES)
def test_pose_gt_info_equals_reference(gold, c):
    d = _case(gold, c)
    out = targets.pose_gt_info(_t(d["cld"]), _t(d["labels"]), _t(d["RT"]), _t(d["model"]), cam_center=_t(d["inv_t"]))
    assert np.array_equal(out["labels"].cpu().numpy(), d["labels_out"])
    assert np.array_equal(out["match_idx"].cpu().numpy(), d["match_idx"])
    assert np.array_equal(out["visible_flag"].cpu().numpy(), d["visible_flag"])
    assert np.array_equal(out["valid"].cpu().numpy(), d["valid"])


def test_case_shapes_cover_the_contract(gold):
    """The golden cases hit every branch: both early returns, unmatched labelled points, the origin inside the hull."""
    b, c, e, a = (_case(gold, k) for k in "bcea")
    assert not b["valid"][0] and (b["labels"] == 0).all() and (b["visible_flag"] == 0).all()
    assert not c["valid"][0] and (c["labels"] > 0).any() and c["visible_flag"].any() and (c["match_idx"] == c["M"]).all()
    assert e["vis_ref"][0].sum() == e["M"] - 1                               # vertices[:-1] dropped a model vertex
    assert ((a["match_idx"] == a["M"]) & (a["labels"] > 0)).any() and a["valid"].all()


def test_strided_cld_rgb_nrm_matches_dense(gold):
    d = _case(gold, "a")
    cld = _t(d["cld"])
    crn = torch.cat([cld.transpose(1, 2), torch.randn(d["B"], 6, cld.shape[1], device="cuda")], dim=1).contiguous()
    a = targets.pose_gt_info(cld, _t(d["labels"]), _t(d["RT"]), _t(d["model"]), cam_center=_t(d["inv_t"]))
    b = targets.pose_gt_info(crn, _t(d["labels"]).to(torch.int64), _t(d["RT"]), _t(d["model"]), cam_center=_t(d["inv_t"]))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_shared_and_per_crop_models_agree_and_crops_are_independent(gold):
    d = _case(gold, "a")
    args = (_t(d["cld"]), _t(d["labels"]), _t(d["RT"]))
    shared = targets.pose_gt_info(*args, _t(d["model"]))
    per = targets.pose_gt_info(*args, _t(np.broadcast_to(d["model"], (d["B"],) + d["model"].shape)))
    for k in shared:
        assert torch.equal(shared[k], per[k]), k
    sel = [4, 1]
    sub = targets.pose_gt_info(_t(d["cld"][sel]), _t(d["labels"][sel]), _t(d["RT"][sel]), _t(d["model"]))
    for k in shared:
        assert torch.equal(shared[k][sel], sub[k]), k


def test_visibility_is_permutation_equivariant(gold):
    d = _case(gold, "a")
    perm = np.random.RandomState(5).permutation(d["M"])
    vis = targets.visible_vertices(_t(d["model"]), _t(d["RT"])).cpu().numpy()
    vp = targets.visible_vertices(_t(d["model"][perm]), _t(d["RT"])).cpu().numpy()
    for b in range(d["B"]):
        # vertices[:-1] drops by index, and the camera is outside the model here, so the origin is a vertex: nothing is dropped
        assert np.array_equal(vp[b], vis[b][perm]), b


def test_hipgraph_replay_is_bit_identical(gold):
    d = _case(gold, "d")
    cld, lab, RT, model = _t(d["cld"]), _t(d["labels"]), _t(d["RT"]), _t(d["model"])
    eager = targets.pose_gt_info(cld, lab, RT, model)
    vis_e, f_e = targets.visible_vertices(model, RT, return_flipped=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        targets.pose_gt_info(cld, lab, RT, model)                         # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = targets.pose_gt_info(cld, lab, RT, model)
        vis_g, f_g = targets.visible_vertices(model, RT, return_flipped=True)
    for _ in range(3):
        for k in out:
            out[k].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(out[k], eager[k]), k
        assert torch.equal(vis_g, vis_e) and torch.equal(f_g, f_e)
    # new inputs in the captured buffers: the replay follows them
    d2 = _case(gold, "d")
    RT.copy_(_t(d2["RT"][[2, 0, 1]]))
    g.replay()
    torch.cuda.synchronize()
    want = targets.pose_gt_info(cld, lab, RT, model)
    for k in want:
        assert torch.equal(out[k], want[k]), k


def test_api_refuses_cpu_tensors_and_bad_shapes():
    RT = torch.eye(4)[:3][None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        targets.visible_vertices(torch.zeros(8, 3), RT)
    with pytest.raises(ValueError, match="M >= 4"):
        targets.visible_vertices(torch.zeros(3, 3, device="cuda"), RT.cuda())
    with pytest.raises(ValueError, match="dist_thresh"):
        targets.pose_gt_info(torch.zeros(1, 16, 3, device="cuda"), torch.zeros(1, 16, device="cuda", dtype=torch.uint8), RT.cuda(),
                             torch.zeros(8, 3, device="cuda"), dist_thresh=0.0)


def test_front_end_origin_labels():
    """make_inputs(mask=...) returns the mask at the chosen pixels with 255 -> 1 (linemod_pbr.py:501-502); without a mask the dict
    is unchanged."""
    from geometric_aware_dense_matching_amd import frontend
    rs = np.random.RandomState(3)
    depth, rgb, nrm = synthetic.make_frame(rs)
    S, N = 256, 1024
    y0, x0 = 100, 200
    mask = np.zeros((480, 640), np.uint8)
    mask[150:220, 250:300] = 255
    mask[230:240, 250:300] = 3
    dev = torch.device("cuda")
    args = (torch.from_numpy(synthetic.normalize_color(rgb).transpose(2, 0, 1)[None].copy()).to(dev), torch.from_numpy(depth[None]).to(dev),
            torch.from_numpy(nrm.transpose(2, 0, 1)[None].copy()).to(dev), torch.from_numpy(synthetic.LM_K[None]).to(dev),
            torch.tensor([[x0, y0]], dtype=torch.int32, device=dev), S, N)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    plain = frontend.make_inputs(*args, generator=gen)
    gen.manual_seed(9)
    inp = frontend.make_inputs(*args, generator=gen, mask=torch.from_numpy(mask[None]).to(dev))
    assert "origin_labels" not in plain and torch.equal(plain["choose"], inp["choose"])
    ch = inp["choose"][0, 0].cpu().numpy()
    want = mask[y0:y0 + S, x0:x0 + S].reshape(-1)[ch].copy()
    want[want == 255] = 1
    got = inp["origin_labels"][0].cpu().numpy()
    assert np.array_equal(got, want) and (got == 1).any() and (got == 3).any()
