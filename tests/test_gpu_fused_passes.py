"""The image branch without three passes over full-resolution maps that no consumer needs:
  * ops.conv64_gather_add_final: the 64-channel point->pixel fusion and `final` behind it in one launch, the fused map never stored;
  * ops.gather_add_affine_act(f32_out=False): the packed operand alone where the next stage's GEMM is the only reader.
Both must give the SAME BITS as the launches they replace (the build runs with -ffp-contract=off and the kernels keep the expressions
and their order), so every comparison here is torch.equal -- no tolerance."""
import ctypes
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as _ops
    return _ops


def _fusion_case(B, m, n, seed, bad_idx=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 64, m, generator=g)
    w = torch.randn(64, 64, generator=g) * 0.2
    t = torch.randn(B, n, 64, generator=g)                        # point-major
    idx = torch.randint(0, n, (B, m), generator=g, dtype=torch.int32)
    if bad_idx:                                                   # the kernels clamp to [0, n - 1]
        idx[:, ::7] = -3
        idx[:, 3::11] = n + 10
        idx[0, 0] = -2 ** 31
        idx[-1, -1] = 2 ** 31 - 1
    sc = torch.rand(64, generator=g) + 0.5
    sh = torch.randn(64, generator=g)
    wf = torch.randn(64, 64, 1, 1, generator=g) * 0.3
    bf = torch.randn(64, generator=g)
    return [v.cuda() for v in (x, w, t, idx, sc, sh, wf, bf)]


def _two_launches(ops, x, wpk, t, idx, sc, sh, act, slope, wf, bf):
    B, _, m = x.shape
    y = ops.conv64_gather_add_act_mfma(x, wpk, t, idx, sc, sh, act, slope, t_point_major=True)
    return ops.conv1x1_logsoftmax(y.view(B, 64, m, 1), wf, bf).view(B, 64, m)


@pytest.mark.gpu
@pytest.mark.parametrize("B,m,n,bad_idx", [
    (16, 128 * 128, 128, False),        # the headline shape: up_fuse_p2r[1] + final at 128 x 128, p2r_up_nei_idx1
    (1, 128 * 128, 128, False),
    (1, 1000, 37, True),                # pixel count not a multiple of the 64-pixel tile, indices out of range
    (3, 77, 5, True),
    (2, 63, 1, True),                   # less than one tile, a single point
    (5, 64 * 9 + 1, 300, False),
])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_fused_fusion_final_equals_the_two_launches(ops, B, m, n, bad_idx, act):
    x, w, t, idx, sc, sh, wf, bf = _fusion_case(B, m, n, seed=1000 + 7 * B + m % 97 + act, bad_idx=bad_idx)
    wpk = ops.pack_rows64(w)
    want = _two_launches(ops, x, wpk, t, idx, sc, sh, act, 0.2, wf, bf)
    got = ops.conv64_gather_add_final(x, wpk, t, idx, sc, sh, act, 0.2, wf, bf)
    torch.cuda.synchronize()
    assert got.shape == want.shape and torch.isfinite(want).all()
    assert torch.equal(got, want), "act %d: %d of %d entries differ, max |d| = %g" % (
        act, int((got != want).sum()), want.numel(), (got - want).abs().max().item())


@pytest.mark.gpu
def test_fused_fusion_final_without_bias_and_with_int64_index(ops):
    x, w, t, idx, sc, sh, wf, _ = _fusion_case(2, 130, 9, seed=5)
    wpk = ops.pack_rows64(w)
    want = _two_launches(ops, x, wpk, t, idx, sc, sh, 1, 0.0, wf, None)
    got = ops.conv64_gather_add_final(x, wpk, t, idx.long().unsqueeze(-1), sc, sh, 1, 0.0, wf, None)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_fused_fusion_final_refuses_other_channel_counts(ops):
    x, w, t, idx, sc, sh, wf, bf = _fusion_case(1, 64, 4, seed=6)
    wpk = ops.pack_rows64(w)
    with pytest.raises(ValueError):
        ops.conv64_gather_add_final(x[:, :32].contiguous(), wpk, t, idx, sc, sh, 1, 0.0, wf, bf)
    with pytest.raises(ValueError):
        ops.conv64_gather_add_final(x, wpk, t.transpose(1, 2).contiguous()[:, :, :3].contiguous(), idx, sc, sh, 1, 0.0, wf, bf)


@pytest.mark.gpu
@pytest.mark.parametrize("C,H,W", [(1024, 32, 32), (256, 64, 64)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_packed_only_gather_add_affine_act_writes_the_same_operand(ops, C, H, W, act):
    """The operand of the form without an fp32 store equals, byte for byte, the one the fp32-writing form produces, and the input
    map is left as it was.  Both forms draw the operand buffer from the same pool, so the first result is copied out and the buffer
    cleared in between."""
    B, n = 16, 128
    g = torch.Generator().manual_seed(C + act)
    x = torch.randn(B, C, H * W, generator=g).cuda()
    t = torch.randn(B, C, n, generator=g).cuda()
    idx = torch.randint(-2, n + 2, (B, H * W), generator=g, dtype=torch.int32).cuda()
    sc = (torch.rand(C, generator=g) + 0.5).cuda()
    sh = torch.randn(C, generator=g).cuda()
    assert ops.packed_out_supported(B, C, H, W)
    x0 = x.clone()
    y, pk = ops.gather_add_affine_act(x.clone(), t, idx, sc, sh, act, 0.2, hw=(H, W))
    want_bytes = pk.buf.clone()
    assert int(want_bytes.count_nonzero()) > want_bytes.numel() // 8      # really written (ReLU and the border leave zeros)
    pk.buf.zero_()                                      # the one-pixel border must be zero; the interior is rewritten in full
    got = ops.gather_add_affine_act(x, t, idx, sc, sh, act, 0.2, hw=(H, W), f32_out=False)
    torch.cuda.synchronize()
    assert isinstance(got, ops.PackedAct) and got.shape == (B, C, H, W)
    assert torch.equal(got.buf, want_bytes)
    assert torch.equal(x, x0)                           # no fp32 store: the input is untouched
    assert not torch.equal(y.view_as(x0), x0)           # (the other form did write in place)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gather_add_affine_act_operand_of_two_images_of_two_chunks(ops, act):
    """B = 2 images of C = 256 channels (two 128-channel chunks): the smallest map on which image b's chunks start at b * nchunk, not
    at b.  The operand of both forms is byte-identical to what the pack kernel makes of the fp32 result."""
    B, C, H, W, n = 2, 256, 8, 32, 50
    g = torch.Generator().manual_seed(40 + act)
    x = torch.randn(B, C, H * W, generator=g).cuda()
    t = torch.randn(B, C, n, generator=g).cuda()
    idx = torch.randint(-2, n + 2, (B, H * W), generator=g, dtype=torch.int32).cuda()
    sc = (torch.rand(C, generator=g) + 0.5).cuda()
    sh = torch.randn(C, generator=g).cuda()
    assert ops.packed_out_supported(B, C, H, W)
    y, pk = ops.gather_add_affine_act(x.clone(), t, idx, sc, sh, act, 0.2, hw=(H, W))
    assert pk is not None and pk.shape == (B, C, H, W)
    mine = pk.buf.clone()                               # the pool may hand the same buffer to the launches below
    pk.buf.zero_()
    only = ops.gather_add_affine_act(x, t, idx, sc, sh, act, 0.2, hw=(H, W), f32_out=False)
    assert torch.equal(only.buf, mine)
    mine2 = only.buf.clone()
    only.buf.zero_()
    assert torch.equal(ops.conv3x3_pack_act(y.view(B, C, H, W).clone()).buf, mine2)


@pytest.mark.gpu
def test_packed_only_needs_a_map_the_operand_is_built_for(ops):
    x = torch.zeros(1, 24, 40, device="cuda")
    t = torch.zeros(1, 24, 3, device="cuda")
    idx = torch.zeros(1, 40, dtype=torch.int32, device="cuda")
    sc = torch.ones(24, device="cuda")
    with pytest.raises(ValueError):
        ops.gather_add_affine_act(x, t, idx, sc, sc, 1, 0.0, hw=(5, 8), f32_out=False)
    with pytest.raises(ValueError):
        ops.gather_add_affine_act(x, t, idx, sc, sc, 1, 0.0, f32_out=False)


@pytest.fixture(scope="module")
def emb_case():
    """FFB6DEmb of the headline model (name-seeded weights) and a batch of 2 with its neighbour pyramid."""
    from geometric_aware_dense_matching_amd import pyramid, synthetic
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    N, M = 2048, 8192
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(G, "geomatch_state.json")))
    sd = synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0)
    model.load_state_dict(sd, strict=False)
    emb = model.pcd_emb.cuda().eval()
    batch = synthetic.make_batch(seed=100, batch=2, n_points=N)
    d = {k: torch.from_numpy(batch[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose")}
    d.update(pyramid.build_pyramid(pyramid.cloud_from_inputs(d["cld_rgb_nrm"]), torch.from_numpy(batch["dpt_xyz"]).cuda()))
    torch.cuda.synchronize()
    return emb, d


@pytest.mark.gpu
@pytest.mark.parametrize("two_stream", [False, True])
def test_embedding_forward_same_bits_with_and_without_the_new_paths(ops, emb_case, monkeypatch, two_stream):
    """FFB6DEmb.forward as it is (fused fusion + final, packed-only fusions in front of up_1 and up_2) against the same forward with
    the former ops sequence put back through a monkeypatch: torch.equal on both returned halves, single-stream and two-stream."""
    from geometric_aware_dense_matching_amd import settings
    emb, d = emb_case
    saved = (settings.USE_SIDE_STREAMS, list(settings.SIDE_PARTS))
    calls = {"final": 0, "packed": 0}
    real_final, real_gaa, real_gmax = ops.conv64_gather_add_final, ops.gather_add_affine_act, ops.gather_max
    on_side = []

    def watch_gmax(feature, idx):
        on_side.append(torch.cuda.current_stream(feature.device) == ops.side_stream(feature.device, 0))
        return real_gmax(feature, idx)

    def count_final(*a, **k):
        calls["final"] += 1
        return real_final(*a, **k)

    def count_gaa(*a, **k):
        if k.get("f32_out", True) is False:
            calls["packed"] += 1
        return real_gaa(*a, **k)

    def old_final(x, wpk, t, idx, sc, sh, act, slope, wf, bf):
        calls["final"] += 1
        return _two_launches(ops, x, wpk, t, idx.reshape(x.shape[0], -1), sc, sh, act, slope, wf, bf)

    def old_gaa(x, t, idx, sc, sh, act=0, slope=0.0, hw=None, f32_out=True):
        if f32_out:
            return real_gaa(x, t, idx, sc, sh, act, slope, hw=hw)
        calls["packed"] += 1
        return real_gaa(x, t, idx, sc, sh, act, slope, hw=hw)[1]

    try:
        settings.USE_SIDE_STREAMS = two_stream
        if two_stream:
            settings.SIDE_PARTS = ["point"]
        with torch.no_grad():
            monkeypatch.setattr(ops, "gather_max", watch_gmax)
            monkeypatch.setattr(ops, "conv64_gather_add_final", count_final)
            monkeypatch.setattr(ops, "gather_add_affine_act", count_gaa)
            new = [v.clone() for v in emb(dict(d), parts=True)]
            torch.cuda.synchronize()
            assert calls == {"final": 1, "packed": 2}, calls           # the step really takes the three new paths
            assert on_side and any(on_side) == two_stream, on_side      # the point lane is side stream 0 exactly when asked for
            calls.update(final=0, packed=0)
            monkeypatch.setattr(ops, "conv64_gather_add_final", old_final)
            monkeypatch.setattr(ops, "gather_add_affine_act", old_gaa)
            old = [v.clone() for v in emb(dict(d), parts=True)]
            torch.cuda.synchronize()
            assert calls == {"final": 1, "packed": 2}, calls
    finally:
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS = saved
    assert torch.isfinite(old[0]).all() and torch.isfinite(old[1]).all()
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])


@pytest.mark.gpu
@pytest.mark.parametrize("off", [None, "USE_MFMA_GEMM", "USE_POINTWISE", "USE_PACKED_PRODUCERS", "USE_SPARSE_FINAL", "USE_FUSED_UPCONV"])
def test_embedding_forward_same_bits_on_one_lane_and_on_two(emb_case, off):
    """The stage loop of FFB6DEmb.forward with its point lane on the current stream and on side stream 0: the same kernels on the same
    operands, so torch.equal on both returned halves -- under the defaults and with each switch off that moves a fusion site to
    another form (USE_POINTWISE off: the point term is a library GEMM, formed on the point lane as well)."""
    from geometric_aware_dense_matching_amd import settings
    emb, d = emb_case
    saved = (settings.USE_SIDE_STREAMS, list(settings.SIDE_PARTS), off and getattr(settings, off))
    out = {}
    try:
        if off:
            setattr(settings, off, False)
        settings.SIDE_PARTS = ["point"]
        for two in (False, True):
            settings.USE_SIDE_STREAMS = two
            with torch.no_grad():
                out[two] = [v.clone() for v in emb(dict(d), parts=True)]
            torch.cuda.synchronize()
    finally:
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS = saved[:2]
        if off:
            setattr(settings, off, saved[2])
    for one, two in zip(out[False], out[True]):
        assert torch.isfinite(one).all() and torch.isfinite(two).all()
        assert torch.equal(one, two), "%s off: %d of %d entries differ, max |d| = %g" % (
            off, int((one != two).sum()), one.numel(), (one - two).abs().max().item())


def test_entry_points_refuse_degenerate_arguments():
    """CPU: host-side validation of the new entry point and of the packed-only form, before any HIP call."""
    from geometric_aware_dense_matching_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    f = lib.gdm_conv64_gather_add_final_hip
    assert f(None, None, None, None, None, None, 1, 1, 64, 1, 0.0, None, None, None, None) != 0
    assert b"NULL" in lib.gdm_last_error()
    assert f(p, p, p, p, p, p, 1, 1, 64, 1, 0.0, None, p, p, None) != 0                 # the `final` weight is not optional
    assert f(p, p, p, p, p, p, 1, 1, 64, 1, 0.0, p, p, None, None) != 0                 # nor the output
    for B, n, m, act in [(0, 1, 64, 1), (-1, 1, 64, 1), (1, 0, 64, 1), (1, -1, 64, 1), (1, 1, 0, 1), (1, 1, -1, 1), (1, 1, 64, 3), (1, 1, 64, -1),
                         (65536, 1, 64, 1), (1, 1, 1 << 31, 1)]:
        assert f(p, p, p, p, p, p, B, n, m, act, 0.0, p, None, p, None) != 0, (B, n, m, act)
        assert b"bad shape" in lib.gdm_last_error()
    g = lib.gdm_gather_add_affine_act2_hip
    assert g(p, p, p, p, p, 1, 128, 1, 32, 1, 0.0, None, None, 0, None) != 0            # neither output
    assert b"NULL" in lib.gdm_last_error()
    assert g(p, p, p, p, p, 1, 24, 1, 32, 1, 0.0, None, p, 32, None) != 0               # packed-only keeps the packed form's shape rules
    assert g(p, p, p, p, p, 0, 128, 1, 32, 1, 0.0, None, p, 32, None) != 0
    assert g(p, p, p, p, p, 1, 128, 1, -1, 1, 0.0, None, p, 32, None) != 0
