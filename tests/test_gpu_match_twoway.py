"""GPU: two-way matching (csrc/gdm_match.hip match_panel_twoway_kernel) and the cycle-consistency pair filter (match_cycle_kernel).

The two-way launch must return the hard path's pairs bit for bit; col_idx / col_sim are held, exactly, to the numpy restatement
(matching.match_twoway_numpy) over the kernel's own similarities -- ops.match(return_sim=True), bit-identical to what the kernel
sees, as tests/test_gpu_match_soft.py relies on -- and, in value, to the fp64 restatement from the raw descriptors within the
project's similarity tolerance 1e-4.  The filter is held bit for bit to pose.cycle_filter_numpy.  Inputs: tests/match_twoway_cases.py."""
import functools

import numpy as np
import pytest
import torch

import match_twoway_cases as mc
from geometric_aware_dense_matching_amd import _lib, infer, matching, ops, pose

pytestmark = pytest.mark.gpu

DELTA = 1e-4                                                            # the project's similarity tolerance
ALL_SHAPES = mc.SHAPES + mc.EXTRA_SHAPES


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(B, N, M):
    scene, model = mc.descriptors(B, N, M)
    return _cuda(scene), _cuda(model)


@functools.lru_cache(maxsize=None)
def _rows(B, N, M, prec):
    scene, model = _case(B, N, M)
    return ops.match_pack2(scene, model, prec)


@functools.lru_cache(maxsize=None)
def _twoway(B, N, M, prec, kind):
    srows, mrows = _rows(B, N, M, prec)
    out = ops.match_twoway_packed(srows, mrows, _cuda(mc.mask(B, N, kind)), B, N, M, prec)
    torch.cuda.synchronize()
    return [t.clone() for t in out]


@functools.lru_cache(maxsize=None)
def _hard(B, N, M, prec):
    srows, mrows = _rows(B, N, M, prec)
    return [t.clone() for t in ops.match_packed(srows, mrows, B, N, M, prec)]


@functools.lru_cache(maxsize=None)
def _sim(B, N, M, prec):
    """The kernel's own similarities, f32[B,N,M] on the host."""
    scene, model = _case(B, N, M)
    return ops.match(scene, model, prec, return_sim=True)[2].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref_from_sim(B, N, M, prec, kind):
    sim, mask = _sim(B, N, M, prec), mc.mask(B, N, kind)
    return [matching.match_twoway_numpy(sim[b], None, mask[b]) for b in range(B)]


@functools.lru_cache(maxsize=None)
def _col_sim_fp64(B, N, M, kind):
    scene, model = mc.descriptors(B, N, M)
    mask = mc.mask(B, N, kind)
    return [matching.match_twoway_numpy(scene[b].T, model, mask[b])["col_sim"] for b in range(B)]


# ---- 1: the hard path's pairs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "empty_crop"])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", ALL_SHAPES)
def test_twoway_launch_returns_the_hard_pairs(B, N, M, prec, kind):
    """(2,70,200): a partial row block spanning two crops and a partial panel; (1,256,256): exactly one of each; (3,128,8193): 33
    panels, the last one column wide; (2,300,513): the crop boundary inside the second row block, N % 32 != 0.  Every row, masked
    or not."""
    two, hard = _twoway(B, N, M, prec, kind), _hard(B, N, M, prec)
    assert torch.equal(two[0], hard[0]) and torch.equal(two[1], hard[1])
    assert two[2].shape == (B, M) and two[3].shape == (B, M) and two[2].dtype == torch.int32 and two[3].dtype == torch.float32


# ---- 2: the numpy restatement over the kernel's own similarities, exactly -------------------------------------------------------------
@pytest.mark.parametrize("kind", mc.MASKS)
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", ALL_SHAPES)
def test_columns_equal_the_restatement_over_the_kernels_similarities(B, N, M, prec, kind):
    """No tolerance and no excluded column: col_idx and col_sim of every crop and vertex, and the rows' pairs as well."""
    bi, bs, ci, cs = [t.cpu().numpy() for t in _twoway(B, N, M, prec, kind)]
    mask = mc.mask(B, N, kind)
    for b, ref in enumerate(_ref_from_sim(B, N, M, prec, kind)):
        assert np.array_equal(ci[b], ref["col_idx"]), (b, int((ci[b] != ref["col_idx"]).sum()))
        assert np.array_equal(cs[b], ref["col_sim"]), b
        assert np.array_equal(bi[b], ref["best_idx"]) and np.array_equal(bs[b], ref["best_sim"]), b
        if not mask[b].any():
            assert (ci[b] == -1).all() and np.isneginf(cs[b]).all()
        else:
            assert (ci[b] >= 0).all() and (mask[b][ci[b]] != 0).all() and np.isfinite(cs[b]).all()
        if mask[b].sum() == 1:
            assert (ci[b] == np.flatnonzero(mask[b])[0]).all()


# ---- 3: fp64 from the raw descriptors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "single_row"])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", mc.SHAPES)
def test_col_sim_vs_fp64_from_the_descriptors(B, N, M, prec, kind):
    """Values only (a near-tie may name another row at the same value): every column of every crop with a masked row within 1e-4."""
    cs = _twoway(B, N, M, prec, kind)[3].cpu().numpy().astype(np.float64)
    mask = mc.mask(B, N, kind)
    worst = 0.0
    for b, want in enumerate(_col_sim_fp64(B, N, M, kind)):
        if mask[b].any():
            worst = max(worst, float(np.abs(cs[b] - want).max()))
    print("max |col_sim - fp64| = %.3g (bound %.3g)" % (worst, DELTA))
    assert worst <= DELTA


# ---- 4: exact ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("d", [1, 4, 32, 128])
def test_duplicated_scene_rows_take_the_lowest_index(prec, d):
    """Rows with (r // d) odd repeat row r - d bit for bit: d = 1 two registers of one lane, d = 4 the two half-waves, d = 32 two waves,
    d = 128 four waves apart.  Under a full mask no column names a copy; with the originals masked out every column names the copy
    of the row it named before, at the same similarity."""
    B, N, M = 1, 256, 512
    scene, model = mc.descriptors(B, N, M, "row ties")
    copy = (np.arange(N) // d) % 2 == 1
    scene[0][:, copy] = scene[0][:, np.flatnonzero(copy) - d]
    srows, mrows = ops.match_pack2(_cuda(scene), _cuda(model), prec)
    full = ops.match_twoway_packed(srows, mrows, torch.ones(B, N, dtype=torch.uint8, device="cuda"), B, N, M, prec)
    upper = ops.match_twoway_packed(srows, mrows, _cuda(copy.astype(np.uint8)[None]), B, N, M, prec)
    ci = full[2].cpu().numpy()[0]
    assert not copy[ci].any() and len(set(ci.tolist())) > 20
    assert torch.equal(upper[2], full[2] + d) and torch.equal(upper[3], full[3])
    assert torch.equal(upper[0], full[0]) and torch.equal(upper[1], full[1])


@pytest.mark.parametrize("prec", [0, 1])
def test_duplicated_model_columns_leave_the_row_rule_as_it_is(prec):
    """Columns 300..511 repeat columns 0..211: the rows' arg-max never lands on a copy (match_packed's rule and bits), and a copy's
    column result is its original's."""
    B, N, M = 1, 256, 512
    scene, model = mc.descriptors(B, N, M, "column ties")
    model[:, 300:] = model[:, :212]
    srows, mrows = ops.match_pack2(_cuda(scene), _cuda(model), prec)
    mask = _cuda(mc.mask(B, N, "random"))
    two = ops.match_twoway_packed(srows, mrows, mask, B, N, M, prec)
    hard = ops.match_packed(srows, mrows, B, N, M, prec)
    assert torch.equal(two[0], hard[0]) and torch.equal(two[1], hard[1]) and bool((two[0] < 300).all())
    assert torch.equal(two[2][:, 300:], two[2][:, :212]) and torch.equal(two[3][:, 300:], two[3][:, :212])


# ---- 5: planted winners -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", [(2, 384, 300), (1, 512, 513)])
def test_planted_winners(B, N, M, prec):
    """Scene row r (counted over the batch) is a copy of model column r mod M.  In-crop rows 0..255 -- the first and the last row of
    every 32-row wave tile, both half-waves, all 8 waves -- are each the lowest planted row of some column, and every column,
    the first and the last of every 32-column accumulator block included, is planted: it must name its lowest planted row in each
    crop (the later copies of that row tie with it exactly)."""
    _, model = mc.descriptors(B, N, M, "planted")
    scene, cols = mc.planted_rows(model, B, N)
    bi, bs, ci, cs = [t.cpu().numpy() for t in ops.match_twoway(_cuda(scene), _cuda(model), torch.ones(B, N, dtype=torch.uint8, device="cuda"),
                                                                prec)]
    assert np.array_equal(bi.reshape(-1), cols)
    for b in range(B):
        mine = cols[b * N:(b + 1) * N]
        for j in range(M):
            rows = np.flatnonzero(mine == j)
            if len(rows):
                assert ci[b, j] == rows[0], (b, j, int(ci[b, j]), rows[:3])
                assert cs[b, j] == bs[b, rows[0]] and cs[b, j] > 0.999
    firsts = {int(ci[0, j]) for j in range(min(M, N))}
    edges = {32 * w + r for w in range(8) for r in (0, 31)}               # the first and the last row of all 8 wave tiles
    halves = {32 * w + r for w in range(8) for r in (3, 4, 27, 28)}       # both half-waves' first and last rows within a tile
    assert edges <= firsts and halves <= firsts


# ---- 6: the same bytes on every launch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", [(2, 300, 513), (5, 40, 100)])
def test_two_launches_and_a_dirty_workspace_give_the_same_bytes(B, N, M, prec):
    srows, mrows = _rows(B, N, M, prec)
    mask = _cuda(mc.mask(B, N, "random"))
    pool = ops.BufferPool()
    with ops.buffer_pool(pool):
        first = [t.clone() for t in ops.match_twoway_packed(srows, mrows, mask, B, N, M, prec)]
        second = [t.clone() for t in ops.match_twoway_packed(srows, mrows, mask, B, N, M, prec)]
        ws = ops._workspace(_lib.lib().gdm_match_twoway_partial_bytes(B, N, M), srows.device)
        ws.fill_(0xFF)
        third = ops.match_twoway_packed(srows, mrows, mask, B, N, M, prec)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), c.view(torch.uint8))
    assert _lib.lib().gdm_match_twoway_partial_bytes(B, N, M) >= _lib.lib().gdm_match_partial_bytes(B, N) + 8 * B * M


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    B, N, M = 2, 70, 200
    srows, mrows = _rows(B, N, M, 0)
    mask = _cuda(mc.mask(B, N, "ones"))
    L = _lib.lib()

    def outs(M_):
        return (torch.full((B, N), 7, dtype=torch.int32, device="cuda"), torch.full((B, N), 7.0, device="cuda"),
                torch.full((B, M_), 7, dtype=torch.int32, device="cuda"), torch.full((B, M_), 7.0, device="cuda"))

    def refused(match, s, m, msk, M_, prec=0, N_=N):
        o = outs(M_)
        part = torch.zeros(max(L.gdm_match_twoway_partial_bytes(B, N, M_), 16), dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.GdmError, match=match):
            _lib.call("gdm_match_twoway_packed_hip", s, m, msk, B, N_, M_, prec, *o, part, part.numel())
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in o) and not bool(part.any())

    big = torch.zeros(L.gdm_match_rows_bytes(16385), dtype=torch.uint8, device="cuda")
    refused(r"rc=-1.*M=16385", srows, big, mask, 16385)
    refused(r"rc=-1.*NULL", srows, mrows, None, M)
    off = torch.zeros(srows.numel() + 16, dtype=torch.uint8, device="cuda")
    refused(r"rc=-1.*16-byte aligned", off[4:4 + srows.numel()], mrows, mask, M)
    refused(r"rc=-1.*16-byte aligned", srows, off[4:4 + mrows.numel()], mask, M)
    refused(r"rc=-1.*precision=2", srows, mrows, mask, M, prec=2)
    refused(r"rc=-1.*bad shape", srows, mrows, mask, M, N_=0)
    cld = torch.zeros(B, 9, N, device="cuda")
    bi, ci = torch.zeros(B, N, dtype=torch.int32, device="cuda"), torch.zeros(B, M, dtype=torch.int32, device="cuda")
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.GdmError, match=r"rc=-1.*radius"):
            ops.match_cycle(cld, bi, ci, mask, bad)
    with pytest.raises(ValueError, match="twoway and soft exclude each other"):
        matching.match_frames(dict(seg=torch.zeros(B, 2, N, device="cuda"), rgbd=_case(B, N, M)[0], mesh=_case(B, N, M)[1]),
                              soft=dict(gamma=16.0, model_xyz=torch.zeros(M, 3, device="cuda")), twoway=True)


# ---- 8: the cycle filter against its restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.0, 0.005])
@pytest.mark.parametrize("N", [1, 70, 257])
def test_match_cycle_equals_its_restatement_bit_for_bit(N, radius):
    """A real [B,9,N] tensor (xyz = its first three rows), an out-of-range best_idx on either side, col_idx = -1 entries and a NaN
    coordinate; N = 257 takes a thread to its second point."""
    B, M = 3, 50
    cld, best_idx, col_idx, mask = mc.cycle_case(B, N, M)
    pm, pc, d2 = [t.cpu().numpy() for t in ops.match_cycle(_cuda(cld), _cuda(best_idx), _cuda(col_idx), _cuda(mask), radius)]
    kept = 0
    for b in range(B):
        wpm, wn, wd2 = pose.cycle_filter_numpy(cld[b, :3].T, best_idx[b], col_idx[b], mask[b], radius)
        assert np.array_equal(pm[b], wpm) and pc[b] == wn, b
        nan = np.isnan(wd2)                                 # a NaN is a NaN: IEEE 754 leaves its sign and payload to the machine
        assert np.array_equal(np.isnan(d2[b]), nan) and np.where(nan, 0, d2[b]).tobytes() == np.where(nan, 0, wd2).tobytes(), b
        kept += wn
    assert pc.dtype == np.int32 and pm.dtype == np.uint8
    if N > 2:
        assert 0 < kept < mask.sum() and np.isnan(d2).any() and np.isposinf(d2[0, 0])
    res = dict(mask=_cuda(mask), best_idx=_cuda(best_idx), col_idx=_cuda(col_idx))
    again = pose.cycle_filter(res, _cuda(cld), radius)
    assert all(a.cpu().numpy().tobytes() == b.tobytes() for a, b in zip(again, (pm, pc, d2)))          # two launches, the same bytes


# ---- 9: the filter does its job ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
def test_cycle_filter_removes_the_planted_outliers(prec):
    """match_twoway_cases.filter_case (tests/test_match_twoway_cpu.py shows on the CPU that it separates exactly): pair_mask is the
    inlier mask, the filtered Kabsch fit is, bit for bit, the fit under the inlier mask, and the unfiltered fit is another."""
    c = mc.filter_case()
    B, _, N = c["scene"].shape
    cld, xyz, inl = _cuda(c["cld"]), _cuda(c["model_xyz"]), _cuda(c["inlier"])
    ones = torch.ones(B, N, dtype=torch.uint8, device="cuda")
    bi, bs, ci, cs = ops.match_twoway(_cuda(c["scene"]), _cuda(c["model"]), ones, prec)
    res = dict(mask=ones, count=ones.sum(1).int(), best_idx=bi, best_sim=bs, col_idx=ci, col_sim=cs)
    pm, pc, d2 = pose.cycle_filter(res, cld, 0.005)
    assert torch.equal(pm, inl) and pc.tolist() == [N - N // 4] * B
    got = pose.estimate_poses(res, cld, xyz, pose_opts=dict(pair_filter="cycle", cycle_radius=0.005))
    want = pose.estimate_poses(dict(res, mask=inl), cld, xyz)
    plain = pose.estimate_poses(res, cld, xyz)
    assert set(got) == {"RT", "valid", "pair_mask", "pair_count"} and set(plain) == {"RT", "valid"}
    assert torch.equal(got["pair_mask"], inl) and torch.equal(got["pair_count"], pc)
    assert torch.equal(got["RT"], want["RT"]) and torch.equal(got["valid"], want["valid"]) and bool(got["valid"].all())
    assert not torch.equal(plain["RT"], got["RT"])
    err = (got["RT"].cpu().numpy() - c["RT"]).__abs__().max()
    err_plain = (plain["RT"].cpu().numpy() - c["RT"]).__abs__().max()
    print("max |RT - truth|: filtered %.3g, unfiltered %.3g" % (err, err_plain))
    assert err < 1e-5 < err_plain
    # the default radius is CYCLE_RADIUS; ransac and consensus see the filtered pairs too, ICP keeps the segmentation mask
    assert torch.equal(pose.estimate_poses(res, cld, xyz, pose_opts=dict(pair_filter="cycle"))["RT"], got["RT"])
    for fit in ("ransac", "consensus"):
        a = pose.estimate_poses(res, cld, xyz, fit, pose_opts=dict(pair_filter="cycle"))
        b = pose.estimate_poses(dict(res, mask=inl), cld, xyz, fit)
        assert torch.equal(a["RT"], b["RT"]) and torch.equal(a["valid"], b["valid"]), fit
    a = pose.estimate_poses(res, cld, xyz, icp_iters=2, pose_opts=dict(pair_filter="cycle"))
    b = pose._icp_stage(dict(RT=got["RT"], valid=got["valid"]), res, cld, xyz, 2, {}, None)
    assert torch.equal(a["RT"], b["RT"]) and torch.equal(a["icp_resid"], b["icp_resid"])


# ---- 10: the pipeline -------------------------------------------------------------------------------------------------------------------
from test_gpu_match_soft import _inputs, c1_model          # noqa: E402,F401  (the C1 model fixture and its seeded crops)

CYCLE_KW = dict(with_pose=True, pose_opts=dict(pair_filter="cycle"))


def test_pipeline_step_with_the_filter(c1_model):          # noqa: F811
    model, d = c1_model, _inputs(61)
    with torch.no_grad():
        base = infer.pipeline_step(model, d, with_pose=True)
        off = infer.pipeline_step(model, d, with_pose=True, match_twoway=False, pose_opts=dict(pair_filter="none"))
        two = infer.pipeline_step(model, d, with_pose=True, match_twoway=True)
        cyc = infer.pipeline_step(model, d, **CYCLE_KW)
        direct = ops.match_twoway(cyc["rgbd"], cyc["mesh"], cyc["mask"], ops.MATCH_BF16X3)
        pm, pc, _ = pose.cycle_filter(cyc, d["cld_rgb_nrm"], pose.CYCLE_RADIUS)
        RT, valid = pose.solve_poses(dict(cyc, mask=pm), d["cld_rgb_nrm"], model.model_emb.xyz)
    assert set(base) == {"seg", "rgbd", "mesh", "mask", "count", "best_idx", "best_sim", "RT", "valid"}      # what it was
    ok, bad = infer.outputs_equal(base, off)
    assert ok and set(base) == set(off), bad
    assert set(two) == set(base) | {"col_idx", "col_sim"} and set(cyc) == set(two) | {"pair_mask", "pair_count"}
    for k in base:
        assert torch.equal(base[k], two[k]), k                                  # the unfiltered fit sees the same pairs
        if k not in ("RT", "valid"):
            assert torch.equal(base[k], cyc[k]), k
    for k, t in zip(("best_idx", "best_sim", "col_idx", "col_sim"), direct):
        assert torch.equal(cyc[k], t) and torch.equal(two[k], t), k
    assert torch.equal(cyc["pair_mask"], pm) and torch.equal(cyc["pair_count"], pc)
    assert torch.equal(cyc["RT"], RT) and torch.equal(cyc["valid"], valid)
    print("masked %d, kept %d" % (int(cyc["count"][0]), int(pc[0])))
    assert int(pc[0]) <= int(cyc["count"][0]) and bool((pm <= cyc["mask"]).all())
    with pytest.raises(ValueError, match="twoway and soft exclude each other"):
        infer.pipeline_step(model, d, with_pose=True, match_gamma=16.0, match_twoway=True)


def test_graphed_pipeline_with_the_filter_replays_the_eager_step(c1_model):          # noqa: F811
    model = c1_model
    gp = infer.GraphedPipeline(model, _inputs(61), forked=False, **CYCLE_KW)
    assert gp.form == "single" and gp.check["single"]["bit_identical"], gp.check
    for seed in (62, 63):
        d = _inputs(seed)
        got = {k: v.clone() for k, v in gp(d).items()}
        with torch.no_grad():
            want = infer.pipeline_step(model, d, **CYCLE_KW)
        ok, bad = infer.outputs_equal(want, got)
        assert ok and set(want) == set(got) and "pair_count" in got, (seed, bad)


def test_run_multi_object_and_test_entry_point_with_the_filter(c1_model, capsys):          # noqa: F811
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    batch = synthetic.make_batch(seed=71, batch=3, n_points=1024)
    d = {k: torch.from_numpy(batch[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
    kw = dict(pose_opts=dict(pair_filter="cycle", cycle_radius=0.01))
    out = infer.run_multi_object({1: c1_model}, d, [1, 1, 1], **kw)
    with torch.no_grad():
        want = infer.pipeline_step(c1_model, d, with_pose=True, **kw)
    for k in ("best_idx", "best_sim", "col_idx", "col_sim", "pair_mask", "pair_count", "RT", "valid"):
        assert torch.equal(out[k], want[k]), k
    argv = ("--gpus=0 -state=test -cls_id=1 --single-object --batch-size 2 --n-points 1024 --n-mesh 512 --synthetic-items 2 "
            "--pair-filter cycle --cycle-radius 0.01").split()
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    assert len(res) == 1 and all("pair_count" in r for r in res)
    kept = train_lm.test.last_kept
    assert len(kept) == 1 and list(kept.values())[0] == [sum(int(r["pair_count"].sum()) for r in res), sum(int(r["count"].sum()) for r in res)]
    assert "--pair-filter cycle (radius 0.01 m): kept fraction" in capsys.readouterr().out


# ---- 11: stream ordering ----------------------------------------------------------------------------------------------------------------
def test_forked_step_with_the_filter_is_ordered():
    """tests/stream_audit.py takes the two-way step as it is: the forked step with the filter on, audited as
    tests/test_gpu_stream_audit.py audits the forked step (two steps, the static inputs overwritten in between).  The point, mesh and
    pyramid forks are there as ever (side streams 0, 1, 2); the mask fork is not taken -- the two-way kernel reads the mask -- so the
    mask, the two-way launch and the filter follow one another on the launch stream."""
    import stream_audit as sa
    import test_gpu_stream_audit as tsa
    from geometric_aware_dense_matching_amd import settings
    model = tsa._ffb6d()
    keys = ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")
    static, other = tsa._crops(131, keys), tsa._crops(132, keys)
    saved = (settings.USE_SIDE_STREAMS, list(settings.SIDE_PARTS), settings.MESH_FORK_LATE)
    pool, launch = ops.BufferPool(), tsa._launch_stream()

    def step(d):
        return infer.pipeline_step(model, d, **CYCLE_KW)

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
    for entry in ("gdm_seg_mask_hip", "gdm_match_twoway_packed_hip", "gdm_match_cycle_hip"):
        assert names.count((entry, "main")) == 2 and sum(1 for n, _ in names if n == entry) == 2, entry
    order = [n for n, _ in names if n in ("gdm_seg_mask_hip", "gdm_match_twoway_packed_hip", "gdm_match_cycle_hip")]
    assert order == ["gdm_seg_mask_hip", "gdm_match_twoway_packed_hip", "gdm_match_cycle_hip"] * 2
    with torch.no_grad():
        single = infer.pipeline_step(model, static, **CYCLE_KW)
    ok, bad = infer.outputs_equal(single, forked)
    assert ok and set(single) == set(forked), bad
