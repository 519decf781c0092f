"""The scene descriptors' matching rows written by the heads kernel itself (gdm_point_heads3_hip, ops.point_heads(rows=True)).

The rows are formed from the kernel's own accumulators by the pack kernel's code (csrc/gdm_match_rows.h: the same partition of the sum
of squares, the same combination, the same division and split), so they are held to the BYTES ops.match_pack writes from the
rgbd_features the same launch stores -- no tolerance -- and rgbd_features / seg to torch.equal with a launch that writes no rows.

Shapes: 64 points per workgroup, so N = 64 (one whole tile), 100 (a partial tile) and 130 (two tiles and two points); the input
given whole (Ca = 128) or as two channel blocks (Ca = 64)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


def _chain(ops, seed, zero=False):
    """The nine layers of GeoMatch's heads with random (or all-zero) weights, folded BatchNorms and biases."""
    rs = np.random.RandomState(seed)
    k = 0.0 if zero else 1.0
    Ws = [torch.from_numpy((k * rs.randn(128, 128) / 11).astype(np.float32)) for _ in range(8)]
    sc = [torch.from_numpy((rs.rand(128) + 0.5).astype(np.float32)) for _ in range(8)]
    sh = [torch.from_numpy((k * rs.randn(128) * 0.3).astype(np.float32)) for _ in range(8)]
    acts = [1, 1, 1, 0, 1, 1, 1, 1]
    sc[3], sh[3] = None, None                                       # the fourth layer: no BN, no bias, no activation
    w_last = torch.from_numpy((rs.randn(2, 128) / 11).astype(np.float32))
    b_last = torch.from_numpy(rs.randn(2).astype(np.float32))
    layers = [(ops.gemm_pack_weight(Ws[l].cuda()), sc[l].cuda() if sc[l] is not None else None,
               sh[l].cuda() if sh[l] is not None else None, acts[l]) for l in range(8)]
    return layers, (ops.gemm_pack_weight(w_last.cuda()), b_last.cuda(), 2)


def _both(ops, x0, Ca, layers, last):
    a = x0[:, :Ca].contiguous()
    b = x0[:, Ca:].contiguous() if Ca < 128 else None
    feat0, seg0 = ops.point_heads(a, b, layers, last, feat_layer=3, res_layer=4)
    feat, seg, rows = ops.point_heads(a, b, layers, last, feat_layer=3, res_layer=4, rows=True)
    rows = rows.clone()                                             # (the buffer belongs to the pool)
    assert rows.dtype == torch.uint8 and rows.numel() == x0.shape[0] * x0.shape[2] * 512
    assert torch.equal(feat, feat0) and torch.equal(seg, seg0), "rgbd_features / seg depend on whether rows are requested"
    want = ops.match_pack(feat, ops.MATCH_BF16X3)
    assert torch.equal(rows, want), "%d of %d row bytes differ from match_pack" % (int((rows != want).sum()), rows.numel())
    return feat, rows


@pytest.mark.parametrize("Ca", [64, 128])
@pytest.mark.parametrize("N", [64, 100, 130])
def test_rows_equal_match_pack_of_the_features(ops, N, Ca):
    B = 2
    layers, last = _chain(ops, N + Ca)
    x0 = torch.from_numpy(np.random.RandomState(N).randn(B, 128, N).astype(np.float32)).cuda()
    feat, _ = _both(ops, x0, Ca, layers, last)
    assert float(feat.abs().max()) > 0.1                           # (descriptors of ordinary size: the norm is no clamp case)


def test_all_zero_features_take_the_clamp(ops):
    """Zero weights and shifts make every feature of every point exactly 0: |x| = 0 is clamped to 1e-12 and the rows are 0 / 1e-12 = 0
    in both halves, as match_pack writes them.  Then zero features for SOME points of a launch whose other points are ordinary."""
    B, N = 2, 100
    layers, last = _chain(ops, 1, zero=True)
    x0 = torch.zeros(B, 128, N, device="cuda")
    feat, rows = _both(ops, x0, 128, layers, last)
    assert not feat.any() and not rows.any()
    # zero inputs for SOME points only: ordinary weights without shifts, the points of crop 0 beyond the 40th are zero
    layers, last = _chain(ops, 2)
    layers = [(w, s, None, a) for (w, s, _sh, a) in layers]
    x0 = torch.from_numpy(np.random.RandomState(3).randn(B, 128, N).astype(np.float32)).cuda()
    x0[0, :, 40:] = 0
    feat, rows = _both(ops, x0, 64, layers, last)
    assert not feat[0, :, 40:].any() and not rows.view(B, N, 512)[0, 40:].any() and rows.view(B, N, 512)[0, :40].any()


def test_rows_need_the_feature_layer(ops):
    from geometric_aware_dense_matching_amd._lib import GdmError
    layers, last = _chain(ops, 4)
    x0 = torch.zeros(1, 128, 64, device="cuda")
    with pytest.raises((GdmError, ValueError)):
        ops.point_heads(x0, None, layers, last, feat_layer=-1, res_layer=4, rows=True)


def test_whole_step_with_both_switches_on_equals_both_off():
    """infer.pipeline_step at B = 2, N = 1024, M = 512 (the neighbour pyramid refuses fewer than 1024 points, so N = 1024 is the
    smallest whole step there is), eager and with the side streams of the forked form: every output tensor with
    settings.SPLINE_LDS_WEIGHTS and settings.HEADS_MATCH_ROWS on equals the step with both off, bit for bit."""
    from geometric_aware_dense_matching_amd import infer, settings, synthetic
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    M = 512
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(G, "geomatch_state.json")))
    model.load_state_dict(synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0), strict=False)
    model = model.cuda().eval()
    b = synthetic.make_batch(seed=83, batch=2, n_points=1024)
    batch = {k: torch.from_numpy(b[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
    saved = (settings.SPLINE_LDS_WEIGHTS, settings.HEADS_MATCH_ROWS, settings.USE_SIDE_STREAMS)
    try:
        for side in (False, True):
            settings.USE_SIDE_STREAMS = side
            outs = []
            for on in (True, False):
                settings.SPLINE_LDS_WEIGHTS = settings.HEADS_MATCH_ROWS = on
                with torch.no_grad():
                    outs.append(infer.pipeline_step(model, dict(batch), with_pose=False))
                torch.cuda.synchronize()
            assert set(outs[0]) == set(outs[1])
            ok, bad = infer.outputs_equal(outs[0], outs[1])
            assert ok, (side, bad)
    finally:
        settings.SPLINE_LDS_WEIGHTS, settings.HEADS_MATCH_ROWS, settings.USE_SIDE_STREAMS = saved
