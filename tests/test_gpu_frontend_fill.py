"""GPU: depth completion (frontend.fill_depth, csrc/gdm_depthfill.hip) against the numpy restatement of its definition
(frontend.fill_depth_numpy, itself held to a scipy composition in test_frontend_fill_cpu.py), and the YCB-V item
(frontend.make_inputs_from_boxes(depth_fill=...)).  Every stage up to the bilateral filter is comparisons, selections and one
subtraction, so it is compared value for value; the bilateral stage multiplies by expf, whose last bit differs between the device's
and numpy's libraries, so the final output has a bound in ulp."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_frontend_boxes import BOXES, H, S, W, _boxes_for, _cuda, _frames  # noqa: E402

from geometric_aware_dense_matching_amd import frontend, synthetic  # noqa: E402

ULP = 2.0 ** -17                                     # one ulp of fp32 in [64, 128): the inverted depths next to max_depth = 100
CASES = synthetic.make_fill_crops()
EXACT = ["s1_inverted_depths", "s2_dilated_depths", "s3_closed_depths", "s4_blurred_depths", "s5_combined_depths",
         "s6_extended_depths", "s7_before_bilateral"]
# max |device - restatement| of the final output over every batch below, in ulp of fp32 at max_depth, measured on an MI355X: 6 ulp
# (the whole frame, fast mode; 5 ulp on the 256 x 256 crops, 0 on the constant block) -- the device's expf and numpy's exp differ in
# the last bit of some weights, and each such weight re-rounds the thirteen products and sums behind it.  Four times that is allowed
# and never more than 13 ulp (0.1 mm; the consumer truncates to millimetres), so 13 it is.
DEVICE_ULP_MEASURED = 6.0
DEVICE_ULP_BOUND = min(4.0 * DEVICE_ULP_MEASURED, 13.0)


def _batch16():
    """Sixteen different 256 x 256 crops: the four named ones and twelve windows of frames with 2 % .. 60 % holes."""
    crops = [CASES[n] for n in ("A", "B", "zero", "sparse")]
    for i in range(12):
        d = synthetic.make_frame(np.random.RandomState(100 + i), hole_frac=0.02 + 0.05 * i)[0]
        y0, x0 = 13 * i, 31 * i
        c = d[y0:y0 + 256, x0:x0 + 256].copy()
        if i % 3 == 0:
            c[:, 40 + i:90 + i] *= np.float32(25.0)              # the medium bin
        if i % 4 == 1:
            c[: 20 + 5 * i, 100:180] = 0                         # an empty top band
        crops.append(c)
    return np.stack(crops)


BATCHES = {"frame": CASES["frame"][None], "odd": CASES["odd"][None], "block": CASES["block"][None], "A": CASES["A"][None],
           "three_256": np.stack([CASES["A"], CASES["B"], CASES["sparse"]]),
           "three_64": np.stack([CASES["small"], CASES["pixel"], CASES["block"]]),
           "sixteen": _batch16()}


@pytest.mark.parametrize("mode", ["multiscale", "fast"])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_stages_equal_the_restatement(name, mode):
    batch = BATCHES[name]
    want_out, want = frontend.fill_depth_numpy(batch, mode=mode, return_stages=True)
    out, st = frontend.fill_depth(_cuda(batch)[0], mode=mode, return_stages=True)
    assert sorted(st) == sorted(want) and out.shape == batch.shape and out.dtype == torch.float32
    for k in EXACT:
        if k in want:
            assert np.array_equal(st[k].cpu().numpy(), want[k]), k
    for k in ("s7_blurred_depths", "s8_inverted_depths"):
        err = np.abs(st[k].cpu().numpy().astype(np.float64) - want[k]).max() / ULP
        print("fill_depth %s %s %s: %.3f ulp" % (name, mode, k, err))
        assert err <= DEVICE_ULP_BOUND, (k, err)
    assert np.array_equal((out > 0.1).cpu().numpy(), want_out > np.float32(0.1))
    # without the stages the same output, bit for bit
    assert torch.equal(frontend.fill_depth(_cuda(batch)[0], mode=mode), out)
    if name == "block" and mode == "multiscale":                 # an empty column has top row 0: the block grows above itself
        assert (out[0, :28] > 0.1).sum().item() == 340


def test_refusals():
    d = _cuda(CASES["small"][None])[0]
    for kw in (dict(extrapolate=True), dict(blur_type="gaussian"), dict(mode="slow")):
        with pytest.raises(ValueError):
            frontend.fill_depth(d, **kw)
    with pytest.raises(ValueError):
        frontend.fill_depth(d[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frontend.fill_depth(d.cpu())
    dirty = CASES["small"][None].copy()
    holes = dirty == 0
    dirty[holes] = np.where(np.arange(holes.sum()) % 2 == 0, np.nan, -1.0)
    assert torch.equal(frontend.fill_depth(_cuda(dirty)[0]), frontend.fill_depth(d))
    got = frontend.fill_depth(d, max_depth=50.0).cpu().numpy()
    want = frontend.fill_depth_numpy(CASES["small"][None], max_depth=50.0)
    assert np.abs(got.astype(np.float64) - want).max() / (ULP / 2) <= DEVICE_ULP_BOUND


def _pyramid_equals_oracle(inp, b, N):
    """Every array of crop b's pyramid against oracle/pyramid.py under the duplicate-point rule: the distances of the
    chosen neighbours are bit-equal row by row and the index sets agree strictly inside the K-th distance."""
    from oracle import knn as oknn
    from oracle import pyramid as opyr
    xyz = inp["dpt_xyz"][b].cpu().numpy()
    cld = inp["cld_rgb_nrm"][b, :3].t().cpu().numpy()
    want = opyr.build_pyramid(cld.copy(), xyz)
    grids = opyr.strided_xyz_grids(xyz, S)
    for key, v in want.items():
        got = inp[key][b].cpu().numpy()
        i = int(key[-1])
        if key.startswith("cld_xyz"):
            assert np.array_equal(got, v), key
            continue
        if key.startswith("cld_sub_idx"):
            assert np.array_equal(got, inp["cld_nei_idx%d" % i][b, : got.shape[0]].cpu().numpy()), key
            continue
        cur, sub = want["cld_xyz%d" % i], want["cld_xyz%d" % i][: N // 4 ** (i + 1)]
        up = want["cld_xyz%d" % (opyr.N_DS - i - 1)] if "_up_" in key else None
        sup, qry = {"cld_nei": (cur, cur), "cld_int": (sub, cur), "r2p_ds": (grids[opyr.RGB_DS_SR[i]], sub),
                    "p2r_ds": (sub, grids[opyr.RGB_DS_SR[i]]), "r2p_up": (grids[opyr.RGB_UP_SR[min(i, 2)]], up),
                    "p2r_up": (up, grids[opyr.RGB_UP_SR[min(i, 2)]])}[key[:6] if key[:3] != "cld" else key[:7]]
        assert got.shape == v.shape and got.min() >= 0 and got.max() < len(sup), (b, key)
        raw_g, raw_w = oknn.d2_of(sup, qry, got), oknn.d2_of(sup, qry, v)
        dg, dw = np.sort(raw_g, axis=1), np.sort(raw_w, axis=1)
        assert np.array_equal(dg, dw), (b, key)
        worst = dg[:, -1:]
        assert np.array_equal(np.sort(np.where(raw_g < worst, got, -1), axis=1),
                              np.sort(np.where(raw_w < worst, v, -1), axis=1)), (b, key)


@pytest.mark.parametrize("mode", ["multiscale", "fast"])
def test_ycbv_item(mode):
    """The six kinds of box; crop first, fill the cropped depth, normals of the filled crop with the frame's K, choose among the
    filled pixels, cld from the UNFILLED dpt_xyz (rows of zeros inside filled holes, as the reference)."""
    B, N = len(BOXES), 2048
    depth, rgb, mask, _, K = _frames(81, B)
    r, d, k, m, bx = _cuda(rgb, depth, K, mask, _boxes_for(BOXES))
    g = torch.Generator(device="cuda").manual_seed(13)
    inp = frontend.make_inputs_from_boxes(r, d, k, bx, S, N, mask=m, generator=g, depth_fill=mode)
    center, scale = frontend.dzi_boxes(bx, (H, W))
    assert torch.equal(inp["center"], center) and torch.equal(inp["scale"], scale)
    crop = frontend.crop_from_boxes(r, d, None, k, center, scale, S, mask=m)
    assert sorted(crop) == ["depth", "dpt_xyz", "mask", "rgb"]
    ref = frontend.crop_from_boxes(r, d, frontend.depth_normals(d, k), k, center, scale, S, mask=m)
    assert all(torch.equal(crop[key], ref[key]) for key in crop)                   # leaving the normals out changes nothing else
    assert torch.equal(inp["rgb"], crop["rgb"]) and torch.equal(inp["dpt_xyz"], crop["dpt_xyz"])
    filled = frontend.fill_depth(crop["depth"], mode=mode)
    assert torch.equal(inp["depth_filled"], filled) and inp["depth_filled"].shape == (B, S, S)
    fl = filled.cpu().numpy()
    valid = fl > np.float32(1e-6)
    assert (valid.reshape(B, -1).sum(1) > (crop["depth"].cpu().numpy() > 1e-6).reshape(B, -1).sum(1)).all()       # it filled something
    assert inp["n_valid"].dtype == torch.int32 and np.array_equal(inp["n_valid"].cpu().numpy(), valid.reshape(B, -1).sum(1))
    g = torch.Generator(device="cuda").manual_seed(13)
    choose = frontend.sample_valid_pixels(crop["dpt_xyz"], N, g, valid=filled > 1e-6)
    assert torch.equal(inp["choose"], choose) and inp["choose"].dtype == torch.int32
    ch = choose[:, 0].cpu().numpy().astype(np.int64)
    nrm = frontend.depth_normals_numpy(fl, K)                                      # of the DEVICE's filled depth: exact by construction
    xyz, rgb_c, msk = crop["dpt_xyz"].cpu().numpy(), crop["rgb"].cpu().numpy(), crop["mask"].cpu().numpy()
    zero_rows = 0
    for b in range(B):
        assert valid[b].reshape(-1)[ch[b]].all() and len(np.unique(ch[b])) == N
        cld = xyz[b].reshape(-1, 3)[ch[b]]
        zero_rows += int((~cld.any(axis=1)).sum())
        full = np.concatenate([cld.T, rgb_c[b].reshape(3, -1)[:, ch[b]], nrm[b].reshape(3, -1)[:, ch[b]]], axis=0)
        assert np.array_equal(inp["cld_rgb_nrm"][b].cpu().numpy(), full), b
        lab = msk[b].reshape(-1)[ch[b]]
        assert np.array_equal(inp["origin_labels"][b].cpu().numpy(), np.where(lab == 255, 1, lab))
    assert zero_rows > 50 * B                                                      # points chosen inside filled holes: xyz = (0,0,0)
    assert np.abs(inp["cld_rgb_nrm"][:, 6:9].cpu().numpy()).sum() > 0
    if mode == "multiscale":
        for b in (0, 2):                                                           # a zoom-in and a zoom-out
            _pyramid_equals_oracle(inp, b, N)
    with pytest.raises(ValueError):
        frontend.make_inputs_from_boxes(r, d, k, bx, S, N, depth_fill=mode, normals=frontend.depth_normals(d, k))
    with pytest.raises(ValueError):
        frontend.sample_valid_pixels(crop["dpt_xyz"], N, valid=(filled > 1e-6).reshape(B, -1))


def test_default_item_is_unchanged():
    """depth_fill=None: key for key the composition the LineMOD item has been, for the same generator."""
    B, N = 4, 2048
    depth, rgb, mask, box, K = _frames(91, B)
    r, d, k, m, bx = _cuda(rgb, depth, K, mask, box)
    g = torch.Generator(device="cuda").manual_seed(17)
    inp = frontend.make_inputs_from_boxes(r, d, k, bx, S, N, mask=m, train=True, generator=g, depth_fill=None)
    g = torch.Generator(device="cuda").manual_seed(17)
    same = frontend.make_inputs_from_boxes(r, d, k, bx, S, N, mask=m, train=True, generator=g)
    assert sorted(inp) == sorted(same) and "depth_filled" not in inp
    assert all(torch.equal(inp[key], same[key]) for key in inp)
    g = torch.Generator(device="cuda").manual_seed(17)
    center, scale = frontend.dzi_boxes(bx, (H, W), train=True, generator=g)
    crop = frontend.crop_from_boxes(r, d, frontend.depth_normals(d, k), k, center, scale, S, mask=m)
    choose = frontend.sample_valid_pixels(crop["dpt_xyz"], N, g)
    ch = choose[:, 0].long()
    cld = torch.gather(crop["dpt_xyz"].reshape(B, S * S, 3), 1, ch[:, :, None].expand(-1, -1, 3))
    pts = [torch.gather(crop[key].reshape(B, 3, S * S), 2, ch[:, None, :].expand(-1, 3, -1)) for key in ("rgb", "normals")]
    lab = torch.gather(crop["mask"].reshape(B, S * S), 1, ch)
    want = dict(rgb=crop["rgb"], dpt_xyz=crop["dpt_xyz"], choose=choose, center=center, scale=scale,
                cld_rgb_nrm=torch.cat([cld.transpose(1, 2)] + pts, dim=1),
                n_valid=(crop["depth"].reshape(B, -1) > 1e-6).sum(1).to(torch.int32),
                origin_labels=torch.where(lab == 255, torch.ones_like(lab), lab))
    want.update(frontend.pyramid.build_pyramid(cld.contiguous(), crop["dpt_xyz"]))
    assert sorted(inp) == sorted(want)
    for key, v in want.items():
        assert inp[key].dtype == v.dtype and torch.equal(inp[key], v), key


def test_fill_and_normals_capture_in_a_hipgraph():
    """fill_depth + depth_normals of the filled crop captured once on one stream, replayed on changed input contents: bit-equal to
    the eager calls, in both modes."""
    B = 3
    Kt = _cuda(np.stack([synthetic.LM_K] * B))[0]

    def case(seed):
        fr = [synthetic.make_frame(np.random.RandomState(seed + i), hole_frac=0.1 + 0.2 * i)[0][50:306, 70:326] for i in range(B)]
        fr[1] = fr[1].copy()
        fr[1][:, 100:104] = 0
        fr[1][:60, 150:] = 0
        return _cuda(np.stack(fr))[0]

    def run(dep):
        out = {}
        for mode in ("multiscale", "fast"):
            out[mode] = frontend.fill_depth(dep, mode=mode)
            out[mode + "_normals"] = frontend.depth_normals(out[mode], Kt)
        return out

    static = case(200)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static)
    for seed in (210, 220):
        new = case(seed)
        static.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        want = run(new)
        for key, v in want.items():
            assert torch.equal(out[key], v), (seed, key)
        assert out["multiscale_normals"].any() and not torch.equal(out["multiscale"], out["fast"])
