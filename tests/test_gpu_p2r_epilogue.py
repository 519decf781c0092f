"""The generic point-to-pixel fusion as ONE launch: ops.conv1x1_packed_gather_add_act (the 1x1 GEMM whose epilogue gathers the point
term, adds it, folds the BatchNorm and activates) against the two launches it replaces, ops.gemm_bf16x3_map followed by
ops.gather_add_affine_act, on the same operands.  The library is built with -ffp-contract=off and the epilogue keeps the pair's
expressions in the pair's order, so every comparison is torch.equal: the fp32 map where one is written, the packed operand byte for
byte.  One case is also held against an fp64 restatement, at the tolerance test_gpu_ops.py::test_gemm_bf16x3 uses for this GEMM.

Shapes: the smallest that reach each branch of the epilogue and of the launcher.
  A  128 -> 128, 2 x 8x32, gn 5: one 256-pixel workgroup per image (the batch offsets of gt and gidx)
  B  256 -> 256, 2 x 8x32, gn 5: two K panels, channel tiles with co0 > 0, packed 16-byte group index > 0 inside the 128-channel chunk
  C  128 -> 192, 1 x 8x32, gn 3: Cout no multiple of the tile (masked rows); the pair writes no packed operand here, nor does the fused call
  D  the two tile widths of the launcher (narrow_tiles of csrc/gdm_conv.hip: 64-channel tiles while pixel tiles x ceil(Cout / 128)
     < 256): A to C are all narrow; 128 -> 256 at 2 x 64x256 has 128 pixel tiles x 2 = 256 and takes the 128-channel-tile instance
  E  as A with gn = 1
  F, G, H  the shapes at which the epilogue gathers from global memory instead of from rows staged in LDS (see SHAPES)
Every crop of A to H holds indices of -1 and of gn (the clamp) and repeated indices (gn is far below the pixel count)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as _ops
    return _ops


def _narrow(B, cout, H, W):
    """narrow_tiles of csrc/gdm_conv.hip for a [B, cout, H, W] result."""
    return cout <= 64 or ((B * H * W + 255) // 256) * ((cout + 127) // 128) < 256


def _case(Cin, Cout, B, H, W, gn, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    t = torch.randn(B, Cout, gn, generator=g)
    idx = torch.randint(0, gn, (B, H * W), generator=g, dtype=torch.int32)
    idx[:, 3::17] = -1                                            # clamped to 0 ...
    idx[:, 5::13] = gn                                            # ... and to gn - 1, in every crop
    sc = torch.rand(Cout, generator=g) + 0.5
    sh = torch.randn(Cout, generator=g)
    return [v.cuda() for v in (x, w, t, idx, sc, sh)]


def _with_operand(ops, x):
    """x as the step hands it on: the fp32 map carrying the packed operand its producer wrote (`_gdm_packed`).  Packed again before
    every call: the pair's second launch may draw the very buffer of its input operand from the pool for its output."""
    x._gdm_packed = ops.conv3x3_pack_act(x)
    return x


def _pair(ops, x, wpk, cout, t, idx, sc, sh, act, f32_out):
    B, _, H, W = x.shape
    xm = ops.gemm_bf16x3_map(_with_operand(ops, x), wpk, cout).view(B, cout, H * W)
    r = ops.gather_add_affine_act(xm, t, idx, sc, sh, act, 0.0, hw=(H, W), f32_out=f32_out)
    torch.cuda.synchronize()
    if not f32_out:
        return None, r.buf.clone()
    return r[0].clone(), (r[1].buf.clone() if r[1] is not None else None)


def _fused(ops, x, wpk, cout, t, idx, sc, sh, act, f32_out, packed_input=False):
    B, _, H, W = x.shape
    src = _with_operand(ops, x)
    assert ops.conv1x1_gather_add_supported(src, cout, act, f32_out=f32_out)
    r = ops.conv1x1_packed_gather_add_act(src._gdm_packed if packed_input else src, wpk, cout, t, idx, sc, sh, act, hw=(H, W), f32_out=f32_out)
    torch.cuda.synchronize()
    if not f32_out:
        assert isinstance(r, ops.PackedAct) and r.shape == (B, cout, H, W)
        return None, r.buf.clone()
    assert r[0].shape == (B, cout, H * W)
    return r[0].clone(), (r[1].buf.clone() if r[1] is not None else None)


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if want is not None:
        assert got.shape == want.shape and got.dtype == want.dtype, what
        assert torch.equal(got, want), "%s: %d of %d entries differ" % (what, int((got != want).sum()), want.numel())


SHAPES = {                       # name: (Cin, Cout, B, H, W, gn, packed operand written, 64-channel tiles)
    "A": (128, 128, 2, 8, 32, 5, True, True),
    "B": (256, 256, 2, 8, 32, 5, True, True),
    "C": (128, 192, 1, 8, 32, 3, False, True),
    "D": (128, 256, 2, 64, 256, 5, True, False),
    # the gathered rows are staged in LDS where a workgroup lies in one image (H*W % 256 == 0) and they fit beside the output tile;
    # A to D do.  The lanes gather from global memory in the other cases:
    "F": (128, 128, 2, 4, 32, 5, True, True),          # two images per workgroup
    "G": (128, 256, 2, 64, 256, 64, True, False),      # 128 rows of 65 floats do not fit behind the 128-channel output tile
    "H": (128, 128, 2, 8, 32, 400, True, True),        # 64 rows of 401 floats do not fit behind the 64-channel output tile
}


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fused_epilogue_equals_the_two_launches(ops, name, act):
    Cin, Cout, B, H, W, gn, packed, narrow = SHAPES[name]
    assert _narrow(B, Cout, H, W) == narrow and ops.packed_out_supported(B, Cout, H, W) == packed
    x, w, t, idx, sc, sh = _case(Cin, Cout, B, H, W, gn, seed=17 * Cin + Cout + act)
    for b in range(B):                                            # every crop: both clamps, and repeats
        assert (idx[b] == -1).any() and (idx[b] == gn).any() and idx[b].unique().numel() < idx[b].numel()
    wpk = ops.gemm_pack_weight(w)
    got_y, got_pk = _fused(ops, x, wpk, Cout, t, idx, sc, sh, act, True)
    want_y, want_pk = _pair(ops, x, wpk, Cout, t, idx, sc, sh, act, True)
    assert torch.isfinite(want_y).all() and (act == 0 or bool((want_y == 0).any()))
    _same(got_y, want_y, "fp32 map")
    _same(got_pk, want_pk, "packed operand beside the fp32 map")
    assert (want_pk is not None) == packed
    if packed:
        assert int(want_pk.count_nonzero()) > want_pk.numel() // 8                    # really written
        _same(_fused(ops, x, wpk, Cout, t, idx, sc, sh, act, False)[1], _pair(ops, x, wpk, Cout, t, idx, sc, sh, act, False)[1],
              "packed operand alone")
        _same(_fused(ops, x, wpk, Cout, t, idx, sc, sh, act, False, packed_input=True)[1], want_pk, "packed operand alone, PackedAct input")
    else:
        assert not ops.conv1x1_gather_add_supported(_with_operand(ops, x), Cout, act, f32_out=False)


def test_single_gathered_column(ops):
    """E: gn = 1 -- every index, whatever its value, clamps to column 0."""
    Cin, Cout, B, H, W = SHAPES["A"][:5]
    x, w, t, idx, sc, sh = _case(Cin, Cout, B, H, W, 1, seed=5)
    wpk = ops.gemm_pack_weight(w)
    got = _fused(ops, x, wpk, Cout, t, idx, sc, sh, 1, True)
    want = _pair(ops, x, wpk, Cout, t, idx, sc, sh, 1, True)
    _same(got[0], want[0], "fp32 map")
    _same(got[1], want[1], "packed operand")


def test_fused_epilogue_against_fp64(ops):
    """Case A against act(scale * (W x + t[idx]) + shift) in fp64, at test_gemm_bf16x3's tolerance: 2e-5 * max(1, max |reference|)."""
    Cin, Cout, B, H, W, gn = SHAPES["A"][:6]
    x, w, t, idx, sc, sh = _case(Cin, Cout, B, H, W, gn, seed=9)
    wpk = ops.gemm_pack_weight(w)
    got = _fused(ops, x, wpk, Cout, t, idx, sc, sh, 1, True)[0].cpu().double()
    mm = torch.matmul(w.cpu().double(), x.cpu().double().view(B, Cin, H * W))
    src = idx.cpu().long().clamp(0, gn - 1).unsqueeze(1).expand(B, Cout, H * W)
    pre = mm + torch.gather(t.cpu().double(), 2, src)
    ref = (sc.cpu().double()[None, :, None] * pre + sh.cpu().double()[None, :, None]).clamp(min=0)
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    print("max |fused - fp64| = %.3e, tolerance %.3e" % (err, tol))
    assert err < tol


def test_gather_add_affine_act_runs_a_pending_gemm_as_one_launch(ops):
    """ops.GemmMap in place of the fp32 map (what FFB6DEmb._p2r_fuse passes): gather_add_affine_act then is the fused call."""
    Cin, Cout, B, H, W, gn = SHAPES["A"][:6]
    x, w, t, idx, sc, sh = _case(Cin, Cout, B, H, W, gn, seed=11)
    wpk = ops.gemm_pack_weight(w)
    want = _fused(ops, x, wpk, Cout, t, idx, sc, sh, 1, True)
    pend = ops.GemmMap(_with_operand(ops, x), wpk, Cout)
    assert pend.shape == (B, Cout, H * W)
    y, pk = ops.gather_add_affine_act(pend, t, idx, sc, sh, 1, 0.0, hw=(H, W))
    torch.cuda.synchronize()
    _same(y, want[0], "fp32 map")
    _same(pk.buf, want[1], "packed operand")
    only = ops.gather_add_affine_act(ops.GemmMap(_with_operand(ops, x), wpk, Cout), t, idx, sc, sh, 1, 0.0, hw=(H, W), f32_out=False)
    torch.cuda.synchronize()
    _same(only.buf, want[1], "packed operand alone")


def test_what_the_fused_call_is_not_built_for(ops):
    Cin, Cout, B, H, W, gn = SHAPES["A"][:6]
    x, w, t, idx, sc, sh = _case(Cin, Cout, B, H, W, gn, seed=13)
    wpk = ops.gemm_pack_weight(w)
    assert not ops.conv1x1_gather_add_supported(x, Cout, 1)                          # no packed operand on the map
    assert not ops.conv1x1_gather_add_supported(_with_operand(ops, x), Cout, 2)      # leaky ReLU: the two launches
    assert not ops.conv1x1_gather_add_supported(_with_operand(ops, x), 64, 1)        # not a GEMM gemm_supported takes
    with pytest.raises(ValueError):
        ops.conv1x1_packed_gather_add_act(x.clone(), wpk, Cout, t, idx, sc, sh, 1, hw=(H, W))        # (the clone carries no operand)
    with pytest.raises(ValueError):
        ops.conv1x1_packed_gather_add_act(_with_operand(ops, x), wpk, Cout, t, idx, sc, sh, 2, hw=(H, W))


def test_embedding_forward_same_bits_as_the_two_launch_path(ops, monkeypatch):
    """FFB6DEmb.forward of the headline model (batch 2) with the four generic fusions as one launch each, against the same forward
    with the predicate turned off (the GEMM and gather_add_affine_act as two launches): torch.equal on both returned halves."""
    import json
    import os
    from geometric_aware_dense_matching_amd import pyramid, synthetic
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    N, M = 2048, 8192
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(golden, "geomatch_state.json")))
    model.load_state_dict(synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0), strict=False)
    emb = model.pcd_emb.cuda().eval()
    batch = synthetic.make_batch(seed=100, batch=2, n_points=N)
    d = {k: torch.from_numpy(batch[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose")}
    d.update(pyramid.build_pyramid(pyramid.cloud_from_inputs(d["cld_rgb_nrm"]), torch.from_numpy(batch["dpt_xyz"]).cuda()))
    calls = []
    real = ops.conv1x1_packed_gather_add_act

    def counted(x, wpk, cout, *a, **k):
        calls.append((cout, k.get("f32_out", True)))
        return real(x, wpk, cout, *a, **k)

    with torch.no_grad():
        monkeypatch.setattr(ops, "conv1x1_packed_gather_add_act", counted)
        new = [v.clone() for v in emb(dict(d), parts=True)]
        torch.cuda.synchronize()
        assert sorted(calls) == [(128, True), (256, False), (512, True), (1024, False)], calls      # the four generic fusion sites
        del calls[:]
        monkeypatch.setattr(ops, "conv1x1_gather_add_supported", lambda *a, **k: False)
        old = [v.clone() for v in emb(dict(d), parts=True)]
        torch.cuda.synchronize()
        assert calls == []
    assert torch.isfinite(old[0]).all() and torch.isfinite(old[1]).all()
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
