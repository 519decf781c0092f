"""GPU parity tests of the HIP operators against the oracle (tests call through the C ABI via
geometric_aware_dense_matching_amd.ops).  Bit-exact for indices and pure data movement; fp32
tolerances are written at each check."""
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from geometric_aware_dense_matching_amd import settings  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


def _cloud(rs, B, n):
    return rs.rand(B, n, 3).astype(np.float32)


@pytest.mark.parametrize("S,Q,K", [(2048, 2048, 16), (512, 2048, 1), (4096, 512, 16), (512, 4096, 1),
                                    (32, 32, 16), (8, 32, 1), (1024, 8, 16), (8, 1024, 1),
                                    (16384, 128, 16), (128, 16384, 1), (1000, 77, 5), (300, 3, 20), (4, 9, 16)])
def test_knn_matches_oracle_bit_exact(ops, S, Q, K):
    from oracle import knn as oknn
    rs = np.random.RandomState(S * 7 + Q)
    B = 2
    sup, qry = _cloud(rs, B, S), _cloud(rs, B, Q)
    want, want_d2 = oknn.knn_batch(sup, qry, K, return_d2=True)
    got, got_d2 = ops.knn_batch(torch.from_numpy(sup).cuda(), torch.from_numpy(qry).cuda(), K, return_d2=True)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(got_d2.cpu().numpy(), want_d2)          # same fp32 arithmetic, no FMA


def test_knn_duplicates_canonical_order(ops):
    """Duplicate points (the loader's np.pad 'wrap'): ties resolved by ascending index, as the oracle."""
    from oracle import knn as oknn
    rs = np.random.RandomState(3)
    base = _cloud(rs, 1, 700)
    sup = np.concatenate([base, base[:, :324]], axis=1)
    want, want_d2 = oknn.knn_batch(sup, sup, 16, return_d2=True)
    got, got_d2 = ops.knn_batch(torch.from_numpy(sup).cuda(), torch.from_numpy(sup).cuda(), 16, return_d2=True)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(got_d2.cpu().numpy(), want_d2)


@pytest.mark.parametrize("case", ["cube", "sheet", "clusters", "line_x", "line_y", "point", "dups", "outside", "k32", "big", "holes", "few"])
def test_knn_cell_list_search_equals_oracle(ops, case):
    """The cell-list search (knn_cells_bin_kernel + knn_cells_kernel: unorganised supports of >= 1024 points through ops.knn_jobs) is
    exact on any data -- indices and (through the oracle's arithmetic) the (d2, index) order bit for bit: a uniform cube (the K-th
    neighbour is often outside the first 3 x 3 cells), a thin depth sheet like a real crop, tight clusters (most cells empty), all points
    on one line (a degenerate axis), one repeated point, exact duplicates (ties by index), queries far outside the support's bounding
    box, K = 32, 16384 points, points at the origin among real ones (depth holes), and a support barely over the threshold with K
    close to the cell population."""
    from oracle import knn as oknn
    rs = np.random.RandomState(zlib.crc32(case.encode()) % (2 ** 31))
    B, S, Q, K = 2, 2048, 1500, 16
    qry = None
    if case == "cube":
        sup = rs.rand(B, S, 3).astype(np.float32)
    elif case == "sheet":
        xy = rs.rand(B, S, 2).astype(np.float32) * 0.3 - 0.15
        z = (0.8 + 0.05 * np.sin(7 * xy[..., :1]) * np.cos(5 * xy[..., 1:])).astype(np.float32)
        sup = np.concatenate([xy, z], axis=2)
    elif case == "clusters":
        c = rs.rand(B, 8, 3).astype(np.float32)
        sup = (c[:, rs.randint(0, 8, S)] + 0.002 * rs.randn(B, S, 3)).astype(np.float32)
    elif case in ("line_x", "line_y"):
        sup = rs.rand(B, S, 3).astype(np.float32)
        sup[..., 0 if case == "line_x" else 1] = 0.25
    elif case == "point":
        sup = np.tile(np.float32([[0.1, -0.2, 0.7]]), (B, S, 1))
    elif case == "dups":
        base = rs.rand(B, 1100, 3).astype(np.float32)
        sup = np.concatenate([base, base[:, :948]], axis=1)
    elif case == "outside":
        sup = rs.rand(B, S, 3).astype(np.float32)
        qry = (rs.rand(B, Q, 3) * 6 - 3).astype(np.float32)
    elif case == "k32":
        sup, K = rs.rand(B, S, 3).astype(np.float32), 32
    elif case == "big":
        S, Q = 16384, 700
        sup = rs.rand(B, S, 3).astype(np.float32)
    elif case == "holes":
        sup = rs.rand(B, S, 3).astype(np.float32) + np.float32([0, 0, 0.5])
        sup[:, rs.rand(S) < 0.1] = 0.0
    else:
        S, Q, K = 1024, 300, 20
        sup = rs.rand(B, S, 3).astype(np.float32)
    if qry is None:
        qry = sup[:, :Q].copy() if case in ("sheet", "dups", "holes") else rs.rand(B, Q, 3).astype(np.float32)
    want = oknn.knn_batch(sup, qry, K)
    (got,) = ops.knn_jobs([(torch.from_numpy(sup).cuda(), torch.from_numpy(qry).cuda(), K)], B)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize("case", ["s512", "s128", "s64", "s1024", "sheet", "dups", "line", "point", "outside", "holes"])
def test_knn1_through_job_table_equals_oracle(ops, case):
    """K = 1 searches through ops.knn_jobs (the pyramid's path: job table + workspace) return the oracle's neighbour -- lowest index
    among equal distances -- on uniform clouds of 64 .. 1024 points, a thin depth sheet queried from its own pixel grid, exact
    duplicates, a degenerate axis, one repeated point, queries far outside the support's box and supports with points at the origin.
    (Written for a cell-list form of the K = 1 search, round 4: exact, but one query per lane walking its own cells is latency-bound --
    147 us against the exhaustive kernel's 73 us per pyramid -- so the exhaustive kernel stays; the cases stay as its test.)"""
    from oracle import knn as oknn
    rs = np.random.RandomState(zlib.crc32(("k1" + case).encode()) % (2 ** 31))
    B, S, Q = 2, 512, 5000
    qry = None
    if case in ("s512", "s128", "s64", "s1024"):
        S = int(case[1:])
        sup = rs.rand(B, S, 3).astype(np.float32)
    elif case == "sheet":
        g = np.stack(np.meshgrid(np.linspace(-0.15, 0.15, 64), np.linspace(-0.15, 0.15, 64)), -1).reshape(-1, 2).astype(np.float32)
        z = (0.8 + 0.05 * np.sin(7 * g[:, :1]) * np.cos(5 * g[:, 1:])).astype(np.float32)
        grid = np.concatenate([g * z / 0.8, z], axis=1)
        qry = np.stack([grid, grid[::-1].copy()])
        sup = np.stack([grid[rs.permutation(4096)[:S]] for _ in range(B)])
    elif case == "dups":
        base = rs.rand(B, 300, 3).astype(np.float32)
        sup = np.concatenate([base, base[:, :212]], axis=1)
        qry = np.concatenate([sup, rs.rand(B, 2000, 3).astype(np.float32)], axis=1)
    elif case == "line":
        sup = rs.rand(B, S, 3).astype(np.float32)
        sup[..., 0] = -0.5
    elif case == "point":
        sup = np.tile(np.float32([[0.3, 0.3, 0.3]]), (B, S, 1))
    elif case == "outside":
        sup = rs.rand(B, S, 3).astype(np.float32)
        qry = (rs.rand(B, Q, 3) * 8 - 4).astype(np.float32)
    else:
        sup = rs.rand(B, S, 3).astype(np.float32) + np.float32([0, 0, 0.5])
        sup[:, rs.rand(S) < 0.15] = 0.0
    if qry is None:
        qry = rs.rand(B, Q, 3).astype(np.float32)
    qry = np.ascontiguousarray(qry, dtype=np.float32)
    want = oknn.knn_batch(sup, qry, 1)
    (got,) = ops.knn_jobs([(torch.from_numpy(np.ascontiguousarray(sup)).cuda(), torch.from_numpy(qry).cuda(), 1)], B)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)


def test_knn_reference_parity_tie_free(ops):
    """Against the REAL reference (nanoflann): its recorded answer (tests/golden/make_golden_knn_ref.py), and the compiled
    reference itself (oracle/_ref) when it is present."""
    from oracle import knn as oknn
    rs = np.random.RandomState(11)
    sup, qry = _cloud(rs, 1, 2048), _cloud(rs, 1, 512)
    want = np.load(os.path.join(os.path.dirname(__file__), "golden", "knn_ref_cases.npz"))["tie_free_K16"].astype(np.int64)
    got = ops.knn_batch(torch.from_numpy(sup).cuda(), torch.from_numpy(qry).cuda(), 16)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    if oknn.have_ref():
        assert np.array_equal(want, oknn.ref_knn_batch(sup, qry, 16))


def test_knn_host_dropin_signature(ops):
    """gdm_knn_batch: host pointers, exact cpp_knn_batch_omp argument list (knn_.h:17-19)."""
    import ctypes
    from geometric_aware_dense_matching_amd import _lib
    from oracle import knn as oknn
    rs = np.random.RandomState(5)
    sup, qry = _cloud(rs, 3, 500), _cloud(rs, 3, 200)
    out = np.zeros((3, 200, 16), dtype=np.int64)
    _lib.lib().gdm_knn_batch(sup.ctypes.data, 3, 500, 3, qry.ctypes.data, 200, 16, out.ctypes.data)
    assert np.array_equal(out, oknn.knn_batch(sup, qry, 16))


def test_knn_jobs_prefix_views(ops):
    from oracle import knn as oknn
    rs = np.random.RandomState(9)
    B = 3
    cld = torch.from_numpy(_cloud(rs, B, 1024)).cuda()
    px = torch.from_numpy(_cloud(rs, B, 4096)).cuda()
    sub = cld[:, :256]
    outs = ops.knn_jobs([(cld, cld, 16), (sub, cld, 1), (px, sub, 16), (sub, px, 1)], B)
    c, s, p = cld.cpu().numpy(), sub.cpu().numpy(), px.cpu().numpy()
    for got, (a, b, k) in zip(outs, [(c, c, 16), (s, c, 1), (p, s, 16), (s, p, 1)]):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), oknn.knn_batch(a, b, k))


def _depth_grid(rs, B, H, W, scale=1.0, holes=0.05, step_edge=True):
    """xyz map [B,H*W,3] of a pinhole depth image: smooth surface + a depth discontinuity + zero holes (points at the origin)."""
    v, u = np.mgrid[:H, :W].astype(np.float32)
    out = np.zeros((B, H * W, 3), np.float32)
    for b in range(B):
        z = 0.8 + 0.1 * np.sin(u / 7.0 + b) * np.cos(v / 5.0) + (rs.rand(H, W).astype(np.float32) - 0.5) * 2e-3
        if step_edge:
            z[:, W // 2:] += 0.35                           # a foreground / background edge
        z[rs.rand(H, W) < holes] = 0.0
        x = (u - W / 2.0 + 0.37) * z / (1.2 * W)
        y = (v - H / 2.0 - 0.21) * z / (1.2 * W)
        out[b] = (np.stack([x, y, z], axis=2) * (z > 0)[:, :, None]).reshape(-1, 3) * scale
    return out


@pytest.mark.parametrize("H,W,K,Q,scale", [(64, 64, 16, 512, 1.0), (128, 128, 16, 128, 1.0), (24, 40, 5, 77, 1.0), (32, 32, 16, 8, 1000.0),
                                           (64, 64, 32, 200, 1.0)])
def test_knn_organised_support_window_search_equals_brute_force(ops, H, W, K, Q, scale):
    """gdm_knn_job.grid_w: the window search over pixel columns / rows (plane bounds from measured x/z, y/z ranges) gives the
    indices and distances of the exhaustive search -- queries on the surface, off the surface, next to the depth edge, behind
    holes; metres and millimetres; grids that are not square."""
    from oracle import knn as oknn
    rs = np.random.RandomState(H * 3 + W + K)
    B = 3
    sup = _depth_grid(rs, B, H, W, scale)
    pick = rs.randint(0, H * W, size=(B, Q))
    qry = np.stack([sup[b][pick[b]] for b in range(B)]) + (rs.randn(B, Q, 3) * 0.003 * scale).astype(np.float32)
    qry[:, : Q // 8] += (rs.randn(B, Q // 8, 3) * 0.2 * scale).astype(np.float32)        # some queries far from the surface
    qry = qry.astype(np.float32)
    want, want_d2 = oknn.knn_batch(sup, qry, K, return_d2=True)
    s_t, q_t = torch.from_numpy(sup).cuda(), torch.from_numpy(qry).cuda()
    got = ops.knn_jobs([(s_t, q_t, K, W)], B)[0].cpu().numpy()
    plain = ops.knn_jobs([(s_t, q_t, K)], B)[0].cpu().numpy()
    # holes are exact duplicates (all at the origin): compare distances, and indices wherever the distance is unique in the list
    d2 = lambda idx: np.stack([oknn.d2_of(sup[b], qry[b], idx[b]) for b in range(B)])
    assert np.array_equal(d2(got), want_d2) and np.array_equal(d2(plain), want_d2)
    assert np.array_equal(got, plain)                                   # canonical (d2, index) order on both paths
    assert np.array_equal(got.astype(np.int64), want)


def test_knn_organised_hint_on_unstructured_data_is_still_exact(ops):
    """The hint is never trusted: a random cloud declared as a grid (ranges wide, no pruning), a map with negative depths (pruning
    switched off for the crop) and an all-hole map give the exhaustive search's result."""
    from oracle import knn as oknn
    rs = np.random.RandomState(5)
    B, H, W, K, Q = 2, 32, 48, 16, 100
    cases = [rs.rand(B, H * W, 3).astype(np.float32) - 0.5, _depth_grid(rs, B, H, W), np.zeros((B, H * W, 3), np.float32)]
    cases[1][:, ::7, 2] *= -1.0
    qry = (rs.rand(B, Q, 3).astype(np.float32) - 0.5)
    for sup in cases:
        want_d2 = oknn.knn_batch(sup, qry, K, return_d2=True)[1]
        got = ops.knn_jobs([(torch.from_numpy(sup).cuda(), torch.from_numpy(qry).cuda(), K, W)], B)[0].cpu().numpy()
        plain = ops.knn_jobs([(torch.from_numpy(sup).cuda(), torch.from_numpy(qry).cuda(), K)], B)[0].cpu().numpy()
        assert np.array_equal(got, plain)
        assert np.array_equal(np.stack([oknn.d2_of(sup[b], qry[b], got[b]) for b in range(B)]), want_d2)


def test_knn_undersized_workspace_takes_the_next_layout_with_the_same_result(ops, monkeypatch):
    """Every rung of the ladder an undersized workspace sends a job down (ranges -> cell list -> hashed tiles -> gather from [S,3]):
    one table with a cell-list support searched by two jobs, an organised 16 x 8 support with holes, a one-tile support and a K = 1
    job -- the smallest shapes that reach every layout -- run with 0 bytes, the full size, 16 bytes less (the tiles of the last
    support no longer fit), room for the first reservation only and for the first two, and room for just the hashed tiles of the
    cell-list support.  The sizes come from the formulas of include/gdm.h.  Indices equal ops.knn_batch on dense copies, bit for bit."""
    rs = np.random.RandomState(41)
    B, H, W = 2, 16, 8
    cell_sup = torch.from_numpy(_cloud(rs, B, 1024)).cuda()
    grid_sup = torch.from_numpy(_depth_grid(rs, B, H, W, holes=0.08, step_edge=False)).cuda()
    assert int((grid_sup[..., 2] == 0).sum()) >= 2                       # a few holes at the origin
    tile_sup = torch.from_numpy(_cloud(rs, B, 77)).cuda()
    q33a, q20, q33b, q33c, q33d = (torch.from_numpy(_cloud(rs, B, n)).cuda() for n in (33, 20, 33, 33, 33))
    q33b = (q33b - 0.5) * 0.2 + torch.tensor([0.0, 0.0, 0.8], device="cuda")          # around the depth surface
    jobs = [(cell_sup, q33a, 5), (cell_sup, q20, 3), (grid_sup, q33b, 5, W), (tile_sup, q33c, 16), (tile_sup, q33d, 1)]
    want = [ops.knn_batch(j[0].contiguous(), j[1].contiguous(), j[2]) for j in jobs]
    cells = B * 1024 * 16 + B * 1036 * 4                                  # reserved first (largest S)
    ranges = (B * (2 * W + 2 * H + 2 * ((H + 15) // 16)) * 4 + 15) // 16 * 16
    tiles = B * 1 * 128 * 16                                              # S = 77: one tile of 128 slots
    full = cells + ranges + tiles
    from geometric_aware_dense_matching_amd import _lib
    for nbytes in (0, full, full - 16, cells, cells + ranges, B * 1 * 1024 * 16):
        seen = []

        def launch(arr, n, B, device, nbytes=nbytes):
            seen.append(int(_lib.lib().gdm_knn_jobs_workspace_bytes(arr, n, B)))
            ws = torch.empty(full, dtype=torch.uint8, device=device)
            ops.call("gdm_knn_jobs_ws_hip", arr, n, B, ws, nbytes)
            return ws

        monkeypatch.setattr(ops, "_knn_launch", launch)
        got = ops.knn_jobs(jobs, B)
        torch.cuda.synchronize()
        assert seen == [full]                                             # the formulas above are the library's
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (nbytes, i)


def _feat_idx(rs, B, C, n, m, K):
    feat = torch.from_numpy(rs.randn(B, C, n).astype(np.float32))
    idx = torch.from_numpy(rs.randint(0, n, size=(B, m, K)).astype(np.int64))
    return feat, idx


@pytest.mark.parametrize("B,C,n,m,K", [(2, 64, 2048, 512, 16), (1, 3, 100, 37, 5), (2, 129, 300, 300, 16), (2, 64, 4096, 128, 16),
                                       (2, 64, 16384, 2048, 16), (1, 5, 1027, 300, 7), (1, 2, 16384, 129, 20), (1, 3, 16385, 200, 16),
                                       (2, 256, 4096, 32, 16), (1, 1024, 1024, 8, 16), (2, 200, 100, 33, 20)])
def test_gather_max(ops, B, C, n, m, K):
    from oracle import ops_ref
    feat, idx = _feat_idx(np.random.RandomState(1), B, C, n, m, K)
    want = ops_ref.random_sample(feat.unsqueeze(3), idx).squeeze(3)
    got = ops.gather_max(feat.cuda(), idx.cuda())
    assert torch.equal(got.cpu(), want)                             # pure selection: bit-exact


@pytest.mark.parametrize("B,C,n,m", [(2, 64, 512, 16384), (1, 7, 33, 100), (2, 256, 32, 1024)])
def test_gather_nn(ops, B, C, n, m):
    from oracle import ops_ref
    feat, idx = _feat_idx(np.random.RandomState(2), B, C, n, m, 1)
    want = ops_ref.nearest_interpolation(feat.unsqueeze(3), idx).squeeze(3)
    got = ops.gather_nn(feat.cuda(), idx.cuda())
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("B,C,n,K", [(2, 16, 2048, 16), (1, 5, 50, 3), (2, 128, 32, 16)])
def test_group_gather(ops, B, C, n, K):
    from oracle import ops_ref
    feat, idx = _feat_idx(np.random.RandomState(3), B, C, n, n, K)
    want = ops_ref.group_gather(feat, idx)
    got = ops.group_gather(feat.cuda(), idx.cuda())
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("B,n,K", [(2, 2048, 16), (1, 40, 16), (3, 128, 4)])
def test_rel_pos_enc(ops, B, n, K):
    from oracle import ops_ref
    rs = np.random.RandomState(4)
    xyz = torch.from_numpy(rs.rand(B, n, 3).astype(np.float32))
    idx = torch.from_numpy(rs.randint(0, n, size=(B, n, K)).astype(np.int64))
    want = ops_ref.relative_pos_encoding(xyz, idx)
    got = ops.rel_pos_enc(xyz.cuda(), idx.cuda()).cpu()
    # channels 1..9 are copies / single subtractions: bit-exact. channel 0 = sqrt of a 3-term sum whose
    # association order inside torch.sum is not specified: 2 ulp.
    assert torch.equal(got[:, 1:], want[:, 1:])
    assert torch.allclose(got[:, 0], want[:, 0], rtol=3e-7, atol=1e-12)


@pytest.mark.parametrize("B,C,n,K", [(2, 32, 2048, 16), (1, 5, 77, 16), (2, 256, 32, 16), (1, 8, 64, 5)])
def test_att_pool(ops, B, C, n, K):
    from oracle import ops_ref
    rs = np.random.RandomState(5)
    att = torch.from_numpy(rs.randn(B, C, n, K).astype(np.float32) * 3)
    feat = torch.from_numpy(rs.randn(B, C, n, K).astype(np.float32))
    want = ops_ref.att_pool_core(att, feat).squeeze(3)
    got = ops.att_pool(att.cuda(), feat.cuda()).cpu()
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)          # exp / summation order


@pytest.mark.parametrize("B,C,n,m,K,extra", [(3, 8, 64, 1024, 1, 5), (2, 16, 256, 256, 16, 16), (2, 6, 50, 77, 1, 3)])
def test_gather_backward_reads_a_channel_slice_in_place(ops, B, C, n, m, K, extra):
    """The gradient a torch.cat backward hands to nearest_interpolation / group_gather is a channel slice of a wider tensor (dense rows,
    larger batch stride): gdm_group_gather_bwd2_hip reads it where it lies -- same result as from a contiguous copy."""
    g = torch.Generator(device="cpu").manual_seed(n + m)
    feat = torch.randn(B, C, n, generator=g).cuda().requires_grad_(True)
    idx = torch.randint(0, n, (B, m, K), generator=g).int().cuda()
    wide = torch.randn(B, C + extra, m, K, generator=g).cuda()
    go = wide[:, extra:]                                              # non-contiguous: batch stride (C + extra) m K
    assert not go.is_contiguous()
    y = ops.group_gather(feat, idx)
    (ga,) = torch.autograd.grad(y, feat, go)
    (gb,) = torch.autograd.grad(ops.group_gather(feat, idx), feat, go.contiguous())
    want = torch.zeros(B, C, n, dtype=torch.float64, device="cuda")
    want.scatter_add_(2, idx.long().view(B, 1, m * K).expand(B, C, m * K), go.reshape(B, C, m * K).double())
    tol = 1e-5 * max(1.0, want.abs().max().item())
    assert (ga.double() - want).abs().max().item() < tol and (gb.double() - want).abs().max().item() < tol


@pytest.mark.parametrize("Cout,Cin,taps", [(128, 256, 9), (64, 128, 9), (128, 200, 1), (512, 64, 1), (128, 128, 9), (256, 72, 9)])
def test_dgrad_weight_pack_equals_pack_of_flipped_transposed_filter(ops, Cout, Cin, taps):
    """gdm_conv_pack_weight_dgrad_hip(w) == pack(w.flip(2, 3).transpose(0, 1)) byte for byte (3x3), == pack(w.t()) (1x1)."""
    g = torch.Generator(device="cpu").manual_seed(Cout + Cin + taps)
    if taps == 9:
        w = torch.randn(Cout, Cin, 3, 3, generator=g).cuda()
        want = ops.conv3x3_pack_weight(w.flip(2, 3).transpose(0, 1).contiguous())
    else:
        w = torch.randn(Cout, Cin, generator=g).cuda()
        want = ops.gemm_pack_weight(w.t().contiguous())
    got = ops.conv_pack_weight_dgrad(w)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("B,C,n,K", [(1, 8, 64, 5), (2, 6, 33, 20), (1, 4, 50, 16)])
def test_att_pool_backward_any_k(ops, B, C, n, K):
    """Att_pooling's softmax . feature . sum over K and its backward for K other than 16 (the general kernels; K = 16 has its own),
    against autograd through the oracle's formulation in fp64."""
    g = torch.Generator(device="cpu").manual_seed(K * 10 + n)
    att = (torch.randn(B, C, n, K, generator=g) * 2).cuda().requires_grad_(True)
    feat = torch.randn(B, C, n, K, generator=g).cuda().requires_grad_(True)
    w = torch.randn(B, C, n, generator=g).cuda()
    (ops.att_pool(att, feat) * w).sum().backward()
    a64, f64 = att.detach().double().requires_grad_(True), feat.detach().double().requires_grad_(True)
    ((torch.softmax(a64, dim=3) * f64).sum(3) * w.double()).sum().backward()
    assert (att.grad.double() - a64.grad).abs().max().item() < 1e-5 * max(1.0, a64.grad.abs().max().item())
    assert (feat.grad.double() - f64.grad).abs().max().item() < 1e-5 * max(1.0, f64.grad.abs().max().item())


def test_gather_backward_matches_autograd(ops):
    from oracle import ops_ref
    rs = np.random.RandomState(6)
    B, C, n, m, K = 2, 24, 200, 150, 16
    feat, idx = _feat_idx(rs, B, C, n, m, K)
    for ref_fn, fn in ((lambda f: ops_ref.random_sample(f.unsqueeze(3), idx).squeeze(3), lambda f: ops.gather_max(f, idx.cuda())),
                       (lambda f: ops_ref.group_gather(f, idx), lambda f: ops.group_gather(f, idx.cuda())),
                       (lambda f: ops_ref.nearest_interpolation(f.unsqueeze(3), idx[:, :, :1]).squeeze(3),
                        lambda f: ops.gather_nn(f, idx[:, :, :1].cuda()))):
        a = feat.clone().requires_grad_(True)
        ya = ref_fn(a)
        w = torch.from_numpy(rs.randn(*ya.shape).astype(np.float32))
        (ya * w).sum().backward()
        b = feat.clone().cuda().requires_grad_(True)
        yb = fn(b)
        (yb * w.cuda()).sum().backward()
        assert torch.allclose(b.grad.cpu(), a.grad, rtol=1e-5, atol=1e-5)   # atomic add order
    att = torch.from_numpy(rs.randn(2, 8, 50, 16).astype(np.float32))
    f = torch.from_numpy(rs.randn(2, 8, 50, 16).astype(np.float32))
    a1, f1 = att.clone().requires_grad_(True), f.clone().requires_grad_(True)
    y = ops_ref.att_pool_core(a1, f1).squeeze(3)
    w = torch.from_numpy(rs.randn(*y.shape).astype(np.float32))
    (y * w).sum().backward()
    a2, f2 = att.clone().cuda().requires_grad_(True), f.clone().cuda().requires_grad_(True)
    (ops.att_pool(a2, f2) * w.cuda()).sum().backward()
    assert torch.allclose(a2.grad.cpu(), a1.grad, rtol=1e-4, atol=1e-6)
    assert torch.allclose(f2.grad.cpu(), f1.grad, rtol=1e-4, atol=1e-6)


def _desc(rs, B, N, M):
    scene = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32) * rs.rand(B, 1, N).astype(np.float32) * 3)
    model = torch.from_numpy(rs.randn(128, M).astype(np.float32))
    return scene, model


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", [(1, 1024, 4096), (2, 2048, 8192), (1, 200, 333), (3, 128, 8193)])
def test_match_vs_oracle(ops, prec, B, N, M):
    """north_star: fp32 similarities within 1e-4 of the reference CPU path. Arg-max: identical index, or a
    different index whose oracle similarity is within the same tolerance of the oracle maximum (near-tie)."""
    from oracle import ops_ref
    scene, model = _desc(np.random.RandomState(N + M), B, N, M)
    gi, gv, gs = ops.match(scene.cuda(), model.cuda(), precision=prec, return_sim=True)
    gi2, gv2 = ops.match(scene.cuda(), model.cuda(), precision=prec)
    gi, gv, gs, gi2, gv2 = gi.cpu(), gv.cpu(), gs.cpu(), gi2.cpu(), gv2.cpu()
    tol = 1e-4
    for b in range(B):
        wv, wi, ws = ops_ref.match_argmax(scene[b], model)
        assert (gs[b] - ws).abs().max().item() < tol
        assert (gv[b] - wv).abs().max().item() < tol
        at_got = ws.gather(1, gi[b].long().unsqueeze(1)).squeeze(1)
        assert ((wv - at_got) < tol).all()
        assert (gi[b].long() == wi).float().mean().item() > 0.999
    # fused (no matrix) and materialising launches agree exactly with each other
    assert torch.equal(gv, gv2) and torch.equal(gi, gi2)
    # and the materialised matrix is consistent with the reported maxima
    assert torch.equal(gs.max(dim=2)[0], gv)


@pytest.mark.parametrize("prec", [0, 1])
def test_match_more_than_64_model_panels(ops, prec):
    """M > 16384 model vertices (more panels than the LDS-panel kernel's grid takes): the tiled kernel + split merge, same contract."""
    from oracle import ops_ref
    N, M = 300, 16384 + 700
    scene, model = _desc(np.random.RandomState(7), 1, N, M)
    gi, gv, gs = ops.match(scene.cuda(), model.cuda(), precision=prec, return_sim=True)
    gi2, gv2 = ops.match(scene.cuda(), model.cuda(), precision=prec)
    wv, wi, ws = ops_ref.match_argmax(scene[0], model)
    assert (gs[0].cpu() - ws).abs().max().item() < 1e-4 and (gv[0].cpu() - wv).abs().max().item() < 1e-4
    at_got = ws.gather(1, gi[0].cpu().long().unsqueeze(1)).squeeze(1)
    assert ((wv - at_got) < 1e-4).all()
    assert torch.equal(gi, gi2) and torch.equal(gv, gv2) and torch.equal(gs.max(dim=2)[0], gv)


@pytest.mark.parametrize("prec", [0, 1])
def test_match_first_max_on_exact_ties(ops, prec):
    """Duplicate model vertices give exactly equal similarities: the lowest index must win (torch.max CPU)."""
    rs = np.random.RandomState(0)
    scene, model = _desc(rs, 1, 256, 512)
    model[:, 300:] = model[:, :212]
    gi, gv = ops.match(scene.cuda(), model.cuda(), precision=prec)
    assert (gi.cpu() < 300).all()
    gi2, gv2, _ = ops.match(scene.cuda(), model.cuda(), precision=prec, return_sim=True)
    assert torch.equal(gi, gi2) and torch.equal(gv, gv2)


@pytest.mark.parametrize("B,N,M", [(1, 256, 256), (2, 1024, 4096), (5, 512, 2304), (16, 2048, 8192)])
def test_match_pipelined_kernels_equal_panel_kernel(ops, B, N, M, monkeypatch):
    """The software-pipelined kernels (default where R % 256 == 0 and M % 256 == 0) run the same products in the same
    order as the plain LDS-panel kernel: indices, maxima and the matrix are bit-identical."""
    scene, model = _desc(np.random.RandomState(B + N + M), B, N, M)
    scene, model = scene.cuda(), model.cuda()
    monkeypatch.setenv("GDM_MATCH_KERNEL", "2")
    ri, rv, rs_ = ops.match(scene, model, precision=0, return_sim=True)
    ri2, rv2 = ops.match(scene, model, precision=0)
    monkeypatch.delenv("GDM_MATCH_KERNEL")
    gi, gv, gs = ops.match(scene, model, precision=0, return_sim=True)
    gi2, gv2 = ops.match(scene, model, precision=0)
    assert torch.equal(ri, gi) and torch.equal(rv, gv) and torch.equal(rs_, gs)
    assert torch.equal(ri2, gi2) and torch.equal(rv2, gv2)
    assert torch.equal(gi, gi2) and torch.equal(gv, gv2)


def test_seg_mask(ops):
    from oracle import ops_ref
    rs = np.random.RandomState(1)
    seg = torch.from_numpy(rs.randn(3, 2, 1000).astype(np.float32))
    seg[0, 1, :10] = seg[0, 0, :10]            # exact ties -> class 0
    mask, count = ops.seg_mask(seg.cuda())
    for b in range(3):
        want = ops_ref.seg_mask(seg[b])
        assert torch.equal(mask[b].cpu().bool(), want)
        assert count[b].item() == int(want.sum())


def test_seg_mask_more_than_65536_points(ops):
    """N > 65536 points per crop: the grid-wide kernel with an atomic count (the per-crop workgroup form covers the product's sizes)."""
    from oracle import ops_ref
    rs = np.random.RandomState(11)
    seg = torch.from_numpy(rs.randn(2, 2, 70001).astype(np.float32))
    mask, count = ops.seg_mask(seg.cuda())
    for b in range(2):
        want = ops_ref.seg_mask(seg[b])
        assert torch.equal(mask[b].cpu().bool(), want) and count[b].item() == int(want.sum())


def test_mfma_probes_run(ops):
    """The two measurement probes behind tools/mfma_probe.py (gdm_mfma_probe_hip, gdm_mfma_probe_lds_hip) launch and finish."""
    from geometric_aware_dense_matching_amd import _lib
    sink = torch.zeros(64 * 512, device="cuda")
    L = _lib.lib()
    assert L.gdm_mfma_probe_hip(64, 30, 1, sink.data_ptr(), None) == 0
    assert L.gdm_mfma_probe_hip(64, 30, 3, sink.data_ptr(), None) == 0
    for rpu in (1, 2, 4):
        assert L.gdm_mfma_probe_lds_hip(64, 16, rpu, sink.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert L.gdm_mfma_probe_hip(64, 31, 1, sink.data_ptr(), None) != 0      # iters must be a multiple of 3: refused, not launched


def test_pointops_ballquery_fps(ops):
    rs = np.random.RandomState(2)
    xyz = rs.rand(2, 500, 3).astype(np.float32)
    new = xyz[:, :64].copy()
    r, ns = 0.2, 8
    got = ops.ballquery(r, ns, torch.from_numpy(xyz).cuda(), torch.from_numpy(new).cuda()).cpu().numpy()
    for b in range(2):
        d = xyz[b][None, :, :] - new[b][:, None, :]
        d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for j in range(64):
            hits = np.nonzero(d2[j] < np.float32(r) * np.float32(r))[0][:ns]
            want = np.full(ns, hits[0] if len(hits) else 0)
            want[:len(hits)] = hits
            assert np.array_equal(got[b, j], want)
    fps = ops.furthestsampling(torch.from_numpy(xyz).cuda(), 32).cpu().numpy()
    for b in range(2):
        temp = np.full(500, 1e10, np.float32)
        last, want = 0, [0]
        for _ in range(31):
            d = xyz[b] - xyz[b][last]
            d2 = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            temp = np.minimum(temp, d2)
            last = int(np.argmax(temp))
            want.append(last)
        assert np.array_equal(fps[b], np.array(want))


def test_cpu_tensor_raises(ops):
    with pytest.raises(RuntimeError):
        ops.knn_batch(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), 1)


@pytest.mark.parametrize("B,C,H,W,OH,OW", [(2, 8, 32, 32, 64, 64), (1, 3, 1, 1, 32, 32), (2, 5, 2, 2, 32, 32), (1, 4, 3, 3, 32, 32),
                                            (1, 4, 6, 6, 32, 32), (1, 2, 128, 128, 256, 256), (1, 3, 7, 5, 13, 18)])
def test_upsample_bilinear_align_corners(ops, B, C, H, W, OH, OW):
    """pspnet.py:26-29,38: the reference op is torch's own bilinear interpolate (CPU here). 1e-6 relative:
    same index/weight arithmetic, different association of the 4-term blend."""
    x = torch.from_numpy(np.random.RandomState(H * W).randn(B, C, H, W).astype(np.float32))
    want = torch.nn.functional.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=True)
    got = ops.upsample_bilinear(x.cuda(), (OH, OW)).cpu()
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    a = x.clone().requires_grad_(True)
    torch.nn.functional.interpolate(a, size=(OH, OW), mode="bilinear", align_corners=True).square().sum().backward()
    b = x.clone().cuda().requires_grad_(True)
    ops.upsample_bilinear(b, (OH, OW)).square().sum().backward()
    assert torch.allclose(b.grad.cpu(), a.grad, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("rows,n,k", [(64, 2048, 16), (7, 8192, 20), (5, 100, 4), (3, 33, 32)])
def test_topk_rows(ops, rows, n, k):
    rs = np.random.RandomState(rows + n)
    s = torch.from_numpy(rs.randn(rows, n).astype(np.float32))
    s[0, : n // 2] = s[0, n // 2: 2 * (n // 2)]            # exact ties: lower column first
    idx, val = ops.topk_rows(s.cuda(), k, return_values=True)
    wv, _ = torch.topk(s, k, dim=-1)
    assert torch.equal(val.cpu(), wv)                       # values: bit-exact, descending
    got = idx.cpu().long()
    assert torch.equal(s.gather(1, got), wv)
    order = np.lexsort((np.arange(n)[None, :].repeat(rows, 0), -s.numpy()), axis=1)[:, :k]
    assert np.array_equal(got.numpy(), order)


def test_edge_feature_and_backward(ops):
    from oracle import dgcnn_ref
    rs = np.random.RandomState(3)
    B, C, n, k = 2, 9, 200, 16
    x = torch.from_numpy(rs.randn(B, C, n).astype(np.float32))
    want = dgcnn_ref.get_graph_feature(x, k, dim9=True)
    idx, _ = dgcnn_ref.knn(x[:, :3], k)
    got = ops.edge_feature(x.cuda(), idx.cuda())
    assert torch.equal(got.cpu(), want)
    a = x.clone().requires_grad_(True)
    w = torch.from_numpy(rs.randn(*want.shape).astype(np.float32))
    xt = a.transpose(2, 1)
    f = xt.reshape(B * n, C)[(idx + torch.arange(B).view(-1, 1, 1) * n).view(-1)].view(B, n, k, C)
    (torch.cat((f - xt.unsqueeze(2), xt.unsqueeze(2).expand(B, n, k, C)), dim=3).permute(0, 3, 1, 2) * w).sum().backward()
    b = x.clone().cuda().requires_grad_(True)
    (ops.edge_feature(b, idx.cuda()) * w.cuda()).sum().backward()
    assert torch.allclose(b.grad.cpu(), a.grad, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 16, 8, 32, 32), (1, 5, 3, 7, 9), (2, 64, 64, 16, 16)])
def test_upconv3x3_gather_equals_conv_after_upsample(ops, B, Cin, Cout, H, W):
    """conv3x3(pad 1)(bilinear_up_x2(x)) + per-channel affine + leaky == low-res 1x1 conv + 9-tap gather."""
    rs = np.random.RandomState(B * 100 + Cin)
    x = torch.from_numpy(rs.randn(B, Cin, H, W).astype(np.float32))
    w = torch.from_numpy((rs.randn(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)).astype(np.float32))
    scale = torch.from_numpy((1 + 0.1 * rs.randn(Cout)).astype(np.float32))
    shift = torch.from_numpy((0.1 * rs.randn(Cout)).astype(np.float32))
    up = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    want = torch.nn.functional.conv2d(up, w, None, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    want = torch.where(want > 0, want, want * 0.25)
    wt = w.permute(2, 3, 0, 1).reshape(9 * Cout, Cin, 1, 1).contiguous()
    z = torch.nn.functional.conv2d(x.cuda(), wt.cuda())
    got = ops.upconv3x3_gather(z, scale.cuda(), shift.cuda(), Cout, (2 * H, 2 * W), ops.ACT_LEAKY, 0.25).cpu()
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,Cin,Cout,H,W,OH,OW", [(2, 8, 4, 16, 16, 20, 20), (1, 6, 5, 9, 12, 12, 31), (2, 4, 3, 8, 8, 8, 8)])
def test_upconv3x3_gather_other_scale_factors(ops, B, Cin, Cout, H, W, OH, OW):
    """Output sizes other than 2H x 2W (scale factors the LDS tile does not fit, incl. 1:1) take the direct kernel: conv3x3(pad 1) of the
    align_corners bilinear resize + affine + ReLU == low-res 1x1 conv + 9-tap gather.  (The C entry point once returned success without
    launching anything on this path.)"""
    rs = np.random.RandomState(OH * 100 + OW)
    x = torch.from_numpy(rs.randn(B, Cin, H, W).astype(np.float32))
    w = torch.from_numpy((rs.randn(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)).astype(np.float32))
    scale = torch.from_numpy((1 + 0.1 * rs.randn(Cout)).astype(np.float32))
    shift = torch.from_numpy((0.1 * rs.randn(Cout)).astype(np.float32))
    up = torch.nn.functional.interpolate(x.double(), size=(OH, OW), mode="bilinear", align_corners=True)
    want = torch.relu(torch.nn.functional.conv2d(up, w.double(), None, padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    wt = w.permute(2, 3, 0, 1).reshape(9 * Cout, Cin, 1, 1).contiguous()
    z = torch.nn.functional.conv2d(x.cuda(), wt.cuda())
    out = ops.upconv3x3_gather(z, scale.cuda(), shift.cuda(), Cout, (OH, OW), ops.ACT_RELU)
    assert (out.cpu().double() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("B,C,H,W,OH,OW", [(2, 3, 16, 16, 20, 20), (1, 2, 9, 12, 12, 31), (2, 4, 8, 8, 16, 16)])
def test_upconv3x3_gather_train_forward_backward_any_scale(ops, B, C, H, W, OH, OW):
    """The differentiable 9-tap gather (training form of PSPUpsample) and its backward for x2 AND other scale factors (the backward's
    direct kernel), against autograd through bilinear resize + shifted sums in fp64."""
    g = torch.Generator(device="cpu").manual_seed(OH + OW)
    z = torch.randn(B, 9 * C, H, W, generator=g).cuda().requires_grad_(True)
    bias = torch.randn(C, generator=g).cuda().requires_grad_(True)
    w = torch.randn(B, C, OH, OW, generator=g).cuda()
    out = ops.upconv3x3_gather_train(z, bias, C, (OH, OW))
    (out * w).sum().backward()
    z64, b64 = z.detach().double().requires_grad_(True), bias.detach().double().requires_grad_(True)
    up = torch.nn.functional.interpolate(z64, size=(OH, OW), mode="bilinear", align_corners=True).view(B, 9, C, OH, OW)
    pad = torch.nn.functional.pad(up, (1, 1, 1, 1))
    ref = sum(pad[:, ky * 3 + kx, :, ky:ky + OH, kx:kx + OW] for ky in range(3) for kx in range(3)) + b64.view(1, -1, 1, 1)
    (ref * w.double()).sum().backward()
    tol = lambda t: 1e-5 * max(1.0, t.abs().max().item())
    assert (out.double() - ref).abs().max().item() < tol(ref)
    assert (z.grad.double() - z64.grad).abs().max().item() < tol(z64.grad)
    assert (bias.grad.double() - b64.grad).abs().max().item() < 1e-4 * max(1.0, b64.grad.abs().max().item())


def test_spline_scalar_kernels_for_odd_channel_counts(ops):
    """SplineConv with a channel count that is not a multiple of 4 takes the one-channel-per-thread kernels (the 16-byte forms need
    C % 4 == 0 and 512 % C == 0): the direct first layer against the dense form, and gdm_spline_pairs_aggregate3_hip against its
    definition out_i = mean_e sum_s basis[e,s] Y[pos[e,s]] + root_i + bias."""
    from geometric_aware_dense_matching_amd import _lib, splinecnn
    torch.manual_seed(4)
    M, C = 700, 10
    pos3 = torch.rand(M, 3, device="cuda")
    ei, ea = splinecnn.build_mesh_graph(pos3, k=4)
    order = torch.argsort(ei[1], stable=True)
    rowptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    rowptr[1:] = torch.cumsum(torch.bincount(ei[1][order], minlength=M), 0).to(torch.int32)
    src, attr = ei[0][order].to(torch.int32).contiguous(), ea[order].contiguous()
    conv = splinecnn.SplineConv(9, C).cuda()
    conv.bias.data.normal_(0, 0.1)
    x = torch.randn(M, 9, device="cuda")
    with torch.enable_grad():
        dense = conv(x, rowptr, src, attr, relu=True).detach()
    with torch.no_grad():
        direct = conv(x, rowptr, src, attr, relu=True)
    assert (dense - direct).abs().max().item() < 1e-5 * max(1.0, dense.abs().max().item())
    # pair aggregation, C = 10
    E = int(rowptr[-1])
    R = 5000
    g = torch.Generator(device="cpu").manual_seed(9)
    Y = torch.randn(R, C, generator=g).cuda()
    pos = torch.randint(0, R, (E, 8), generator=g).int().cuda()
    basis = torch.rand(E, 8, generator=g).cuda()
    root = torch.randn(M, C, generator=g).cuda()
    out = torch.empty(M, C, device="cuda")
    rc = _lib.lib().gdm_spline_pairs_aggregate3_hip(Y.data_ptr(), rowptr.data_ptr(), pos.data_ptr(), basis.data_ptr(), root.data_ptr(),
                                                    conv.bias.data_ptr(), M, C, 1, out.data_ptr(), None, None, None)
    assert rc == 0
    msg = (basis.double().unsqueeze(2) * Y.double()[pos.long()]).sum(1)                   # [E, C]
    tgt = torch.repeat_interleave(torch.arange(M, device="cuda"), (rowptr[1:] - rowptr[:-1]).long())
    acc = torch.zeros(M, C, dtype=torch.float64, device="cuda").index_add_(0, tgt, msg)
    deg = (rowptr[1:] - rowptr[:-1]).double().clamp(min=1).unsqueeze(1)
    want = torch.relu(acc / deg + root.double() + conv.bias.double())
    assert (out.double() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 128, 128, 32, 32), (1, 256, 512, 32, 32), (3, 512, 128, 8, 32), (2, 128, 256, 5, 64)])
def test_conv3x3_bf16x3_vs_fp32_conv(ops, B, Cin, Cout, H, W):
    """Split-bf16 MFMA implicit GEMM vs the fp64 convolution on the CPU; error bound 3*2^-16 * sum|w x| per output
    (a bf16 half-ulp is 2^-8 relative: |lo| <= 2^-8 |v|, residual <= 2^-16 |v|, three such terms per product; measured ~1e-6 relative to the output scale), far inside the network tolerance used against the golden vectors."""
    rs = np.random.RandomState(Cin + Cout + H)
    x = torch.from_numpy(rs.randn(B, Cin, H, W).astype(np.float32))
    w = torch.from_numpy((rs.randn(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)).astype(np.float32))
    scale = torch.from_numpy((1 + 0.1 * rs.randn(Cout)).astype(np.float32))
    shift = torch.from_numpy((0.1 * rs.randn(Cout)).astype(np.float32))
    res = torch.from_numpy(rs.randn(B, Cout, H, W).astype(np.float32))
    ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    wpk = ops.conv3x3_pack_weight(w.cuda())
    got = ops.conv3x3_bf16x3(x.cuda(), wpk, Cout).cpu()
    assert (got.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    want2 = torch.relu(ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double())
    got2 = ops.conv3x3_bf16x3(x.cuda(), wpk, Cout, scale.cuda(), shift.cuda(), ops.ACT_RELU, res.cuda()).cpu()
    assert (got2.double() - want2).abs().max().item() < 2e-5 * max(1.0, want2.abs().max().item())
    # a second call reuses the cached zero-bordered buffer: borders must still be zero
    got3 = ops.conv3x3_bf16x3(x.cuda(), wpk, Cout).cpu()
    assert torch.equal(got, got3)


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 64, 64, 64, 64), (1, 64, 128, 8, 32), (2, 128, 64, 4, 32), (1, 256, 200, 8, 32)])
def test_conv3x3_bf16x3_small_channel_counts(ops, B, Cin, Cout, H, W):
    """Cin = 64 (one half-filled 128-channel chunk: the 64 x 64 stage of the trunk) and output channel counts that are not multiples
    of 128 (zero weight rows, masked stores), against the fp64 convolution."""
    rs = np.random.RandomState(Cin * 3 + Cout)
    x = torch.from_numpy(rs.randn(B, Cin, H, W).astype(np.float32))
    w = torch.from_numpy((rs.randn(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)).astype(np.float32))
    assert ops.conv3x3_supported(x.cuda(), w.cuda())
    ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    got = ops.conv3x3_bf16x3(x.cuda(), ops.conv3x3_pack_weight(w.cuda()), Cout).cpu()
    assert (got.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("B,C1,C2,C3,H,W", [(2, 128, 256, 256, 32, 32), (1, 64, 64, 64, 64, 64), (1, 128, 64, 72, 8, 32), (2, 256, 128, 200, 4, 32),
                                            (2, 128, 256, 128, 8, 32)])
def test_conv3x3_packed_output_feeds_the_next_convolution(ops, B, C1, C2, C3, H, W):
    """The epilogue's packed output (bf16 hi / lo planes written straight from the accumulators) == packing the fp32 result with
    the pack kernel, bit for bit, so conv -> conv through it equals conv -> pack -> conv exactly; with and without the fp32 map."""
    rs = np.random.RandomState(C1 + C2 + C3)
    x = torch.from_numpy(rs.randn(B, C1, H, W).astype(np.float32)).cuda()
    w1 = torch.from_numpy((rs.randn(C2, C1, 3, 3) / np.sqrt(C1 * 9)).astype(np.float32)).cuda()
    w2 = torch.from_numpy((rs.randn(C3, C2, 3, 3) / np.sqrt(C2 * 9)).astype(np.float32)).cuda()
    sc = torch.from_numpy((1 + 0.1 * rs.randn(C2)).astype(np.float32)).cuda()
    sh = torch.from_numpy((0.1 * rs.randn(C2)).astype(np.float32)).cuda()
    res = torch.from_numpy(rs.randn(B, C2, H, W).astype(np.float32)).cuda()
    p1, p2 = ops.conv3x3_pack_weight(w1), ops.conv3x3_pack_weight(w2)
    mid = ops.conv3x3_bf16x3(x, p1, C2, sc, sh, ops.ACT_RELU, res)
    want = ops.conv3x3_bf16x3(mid, p2, C3)
    mid_f32, mid_pk = ops.conv3x3_bf16x3(x, p1, C2, sc, sh, ops.ACT_RELU, res, out_packed=True)
    assert torch.equal(mid_f32, mid) and isinstance(mid_pk, ops.PackedAct) and mid_pk.shape == (B, C2, H, W)
    got = ops.conv3x3_bf16x3(mid_pk, p2, C3)
    assert torch.equal(got, want)
    none_f32, only_pk = ops.conv3x3_bf16x3(x, p1, C2, sc, sh, ops.ACT_RELU, res, out_f32=False, out_packed=True)
    assert none_f32 is None and torch.equal(ops.conv3x3_bf16x3(only_pk, p2, C3), want)
    # the pooled operand buffers keep their zero border over repeated use
    for _ in range(3):
        _, pk = ops.conv3x3_bf16x3(x, p1, C2, sc, sh, ops.ACT_RELU, res, out_f32=False, out_packed=True)
        assert torch.equal(ops.conv3x3_bf16x3(pk, p2, C3), want)
    mine = pk.buf.clone()                                         # the pool may hand the same buffer to the pack launch below
    assert torch.equal(ops.conv3x3_pack_act(mid).buf, mine)


@pytest.mark.parametrize("B,C,H,W", [(2, 136, 3, 16), (1, 64, 2, 32)])
def test_pack_kernel_against_the_layout_restated_in_numpy(ops, B, C, H, W):
    """conv3x3_pack_act, the kernel every producer's packed bytes are compared with, against tests/packed_layout.py: the documented
    address of every granule and gdm_split2's round-to-nearest-even hi / lo split, byte for byte (border and unused planes zero).
    The library packs maps of 64 or a multiple of 128 channels; the 136-channel map -- a partial second chunk -- goes in with its
    missing channels as zeros, which by the layout's definition are the same bytes: a plane nobody writes is zero, and so are the hi
    and lo parts of 0.0."""
    import packed_layout as P
    rs = np.random.RandomState(B * 1000 + C)
    x = rs.randn(B, C, H, W).astype(np.float32)
    x[0, 0, 0, :4] = [0.0, -0.0, 1.0 + 2.0 ** -8, 3.0e38]         # zeros, a rounding tie, the top of the range
    want = P.pack(x)
    Cp = C if C == 64 else (C + 127) // 128 * 128
    xp = np.zeros((B, Cp, H, W), np.float32)
    xp[:, :C] = x
    assert want.size == P.packed_bytes(B, Cp, H, W)
    got = ops.conv3x3_pack_act(torch.from_numpy(xp).cuda())
    assert got.shape == (B, Cp, H, W) and got.buf.numel() == want.size
    assert np.array_equal(got.buf.cpu().numpy(), want)


def test_final_stage_and_psp_pools(ops):
    rs = np.random.RandomState(12)
    x = torch.from_numpy(rs.randn(2, 64, 40, 24).astype(np.float32))
    w = torch.from_numpy((rs.randn(64, 64, 1, 1) / 8).astype(np.float32))
    b = torch.from_numpy((0.1 * rs.randn(64)).astype(np.float32))
    want = torch.log_softmax(torch.nn.functional.conv2d(x, w, b), dim=1)
    got = ops.conv1x1_logsoftmax(x.cuda(), w.cuda(), b.cuda()).cpu()
    assert torch.allclose(got, want, rtol=1e-5, atol=2e-5)
    f = torch.from_numpy(rs.randn(3, 7, 32, 32).astype(np.float32))
    outs = ops.psp_pools(f.cuda())
    for s_, o in zip((1, 2, 3, 6), outs):
        assert torch.allclose(o.cpu(), torch.nn.functional.adaptive_avg_pool2d(f, s_), rtol=1e-5, atol=1e-6)
    f2 = torch.from_numpy(rs.randn(1, 3, 13, 9).astype(np.float32))                 # uneven bins
    for s_, o in zip((1, 2, 3, 6), ops.psp_pools(f2.cuda())):
        assert torch.allclose(o.cpu(), torch.nn.functional.adaptive_avg_pool2d(f2, s_), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("B,Cin,Cout,n", [(2, 128, 256, 1024), (1, 1024, 2304, 1024), (1, 128, 16000, 8192), (2, 256, 576, 4096), (1, 128, 200, 64), (2, 64, 576, 4096), (1, 64, 128, 96),
                                          (16, 1024, 2304, 1024), (16, 256, 576, 4096)])      # the step's two tap GEMMs: 144-channel tiles
def test_gemm_bf16x3(ops, B, Cin, Cout, n):
    rs = np.random.RandomState(Cin + n)
    x = torch.from_numpy(rs.randn(B, Cin, n).astype(np.float32))
    w = torch.from_numpy((rs.randn(Cout, Cin) / np.sqrt(Cin)).astype(np.float32))
    ref = torch.matmul(w.double(), x.double())
    wpk = ops.gemm_pack_weight(w.cuda())
    got = ops.gemm_bf16x3(x.cuda(), wpk, Cout).cpu()
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    assert (got.double() - ref).abs().max().item() < tol
    if Cin != 64:        # the 64-channel (half-chunk) form is built for NCHW output only
        got_pm = ops.gemm_bf16x3(x.cuda(), wpk, Cout, pixel_major=True).cpu().view(B, n, Cout).transpose(1, 2)
        assert (got_pm.double() - ref).abs().max().item() < tol


@pytest.mark.parametrize("act", [0, 1, 2])
def test_conv1x1_gather_add_act(ops, act):
    """64-channel point->pixel fusion tail in one pass == GEMM + gather + add + affine + activation in torch (fp64)."""
    rs = np.random.RandomState(act)
    B, C, m, n = 2, 64, 1000, 37
    x = torch.from_numpy(rs.randn(B, C, m).astype(np.float32))
    w = torch.from_numpy((rs.randn(C, C) / 8).astype(np.float32))
    t = torch.from_numpy(rs.randn(B, C, n).astype(np.float32))
    idx = torch.from_numpy(rs.randint(0, n, (B, m)).astype(np.int32))
    scale = torch.from_numpy(rs.rand(C).astype(np.float32) + 0.5)
    shift = torch.from_numpy(rs.randn(C).astype(np.float32))
    pre = torch.matmul(w.double(), x.double()) + torch.gather(t.double(), 2, idx.long().unsqueeze(1).expand(B, C, m))
    ref = scale.double()[None, :, None] * pre + shift.double()[None, :, None]
    if act == 1:
        ref = ref.clamp(min=0)
    if act == 2:
        ref = torch.where(ref > 0, ref, ref * 0.2)
    got = ops.conv1x1_gather_add_act(x.cuda(), w.t().contiguous().cuda(), t.cuda(), idx.cuda(), scale.cuda(), shift.cuda(), act, 0.2).cpu()
    assert (got.double() - ref).abs().max().item() < 2e-5
    got_pm = ops.conv1x1_gather_add_act(x.cuda(), w.t().contiguous().cuda(), t.cuda(), idx.cuda(), scale.cuda(), shift.cuda(), act, 0.2,
                                        pixel_major=True).cpu()
    assert got_pm.shape == (B, m, C) and torch.equal(got_pm.transpose(1, 2), got)          # same arithmetic, other layout
    # the same fusion with the channel mix on split-bf16 MFMA (the default in the model): both layouts, ragged m
    wpk = ops.pack_rows64(w.cuda())
    tol = 3e-5 * max(1.0, ref.abs().max().item())
    got_mm = ops.conv64_gather_add_act_mfma(x.cuda(), wpk, t.cuda(), idx.cuda(), scale.cuda(), shift.cuda(), act, 0.2).cpu()
    assert (got_mm.double() - ref).abs().max().item() < tol
    got_mm_pm = ops.conv64_gather_add_act_mfma(x.cuda(), wpk, t.cuda(), idx.cuda(), scale.cuda(), shift.cuda(), act, 0.2, pixel_major=True).cpu()
    assert got_mm_pm.shape == (B, m, C) and torch.equal(got_mm_pm.transpose(1, 2), got_mm)
    got_tpm = ops.conv64_gather_add_act_mfma(x.cuda(), wpk, t.transpose(1, 2).contiguous().cuda(), idx.cuda(), scale.cuda(), shift.cuda(), act, 0.2,
                                             t_point_major=True).cpu()
    assert torch.equal(got_tpm, got_mm)                              # the point term point-major: same values, one row per gathered point


@pytest.mark.parametrize("B,H,W,N", [(2, 16, 24, 100), (1, 128, 128, 2048), (3, 9, 7, 33)])
def test_upconv_final_points_equals_dense_stage_at_the_chosen_pixels(ops, B, H, W, N):
    """The last image stage (PSPUpsample(64 -> 64) + Conv1x1 + LogSoftmax, /root/reference/models/cnn/pspnet.py:34-45,108-112) evaluated at
    the `choose` pixels only == the stage on the whole 2x map in torch fp64, gathered (ffb6d.py:266-285).  Chosen pixels include all
    four corners and the borders (zero padding of the 3x3, clamped bilinear neighbours), duplicates, and a ragged last block."""
    rs = np.random.RandomState(B * 1000 + N)
    OH, OW = 2 * H, 2 * W
    x = torch.from_numpy(rs.randn(B, 64, H, W).astype(np.float32))
    w3 = torch.from_numpy((rs.randn(64, 64, 3, 3) * 0.05).astype(np.float32))
    scale = torch.from_numpy(rs.rand(64).astype(np.float32) + 0.5)
    shift = torch.from_numpy(rs.randn(64).astype(np.float32))
    wf = torch.from_numpy((rs.randn(64, 64) / 8).astype(np.float32))
    bf = torch.from_numpy(rs.randn(64).astype(np.float32))
    choose = rs.randint(0, OH * OW, size=(B, N)).astype(np.int32)
    choose[:, :6] = [0, OW - 1, (OH - 1) * OW, OH * OW - 1, OW // 2, (OH - 1) * OW + 3]
    choose[:, 6] = choose[:, 7]
    up = torch.nn.functional.interpolate(x.double(), size=(OH, OW), mode="bilinear", align_corners=True)
    h = torch.nn.functional.conv2d(up, w3.double(), padding=1) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    h = torch.where(h > 0, h, 0.25 * h)
    y = torch.einsum("oc,bchw->bohw", wf.double(), h) + bf.double()[None, :, None, None]
    ref = torch.log_softmax(y, dim=1).reshape(B, 64, -1)
    ref = torch.gather(ref, 2, torch.from_numpy(choose).long()[:, None, :].expand(B, 64, N))
    x_pm = x.reshape(B, 64, H * W).transpose(1, 2).contiguous().cuda()
    got = ops.upconv_final_points(x_pm, (H, W), torch.from_numpy(choose).cuda(), ops.upconv_fused64_pack_weight(w3.cuda()), scale.cuda(),
                                  shift.cuda(), 2, 0.25, ops.pack_rows64(wf.cuda()), bf.cuda(), (OH, OW)).cpu()
    assert got.shape == (B, 64, N)
    assert (got.double() - ref).abs().max().item() < 5e-5 * max(1.0, ref.abs().max().item())
    got_nobias = ops.upconv_final_points(x_pm, (H, W), torch.from_numpy(choose).cuda(), ops.upconv_fused64_pack_weight(w3.cuda()),
                                         scale.cuda(), shift.cuda(), 1, 0.0, ops.pack_rows64(wf.cuda()), None, (OH, OW)).cpu()
    ref1 = torch.log_softmax(torch.einsum("oc,bchw->bohw", wf.double(), torch.nn.functional.conv2d(up, w3.double(), padding=1).mul(
        scale.double()[None, :, None, None]).add(shift.double()[None, :, None, None]).clamp(min=0)), dim=1).reshape(B, 64, -1)
    ref1 = torch.gather(ref1, 2, torch.from_numpy(choose).long()[:, None, :].expand(B, 64, N))
    assert (got_nobias.double() - ref1).abs().max().item() < 5e-5 * max(1.0, ref1.abs().max().item())


@pytest.mark.parametrize("d_out,n", [(32, 100), (64, 257), (128, 64), (256, 33)])
def test_fused_lfa_stage_equals_unfused_block(ops, d_out, n):
    """Building_block (RandLANet.py:700-718) as two fused attentive-pooling launches == the gather / GEMM / softmax-pool chain
    of separate kernels (itself pinned against the reference's golden block outputs)."""
    from geometric_aware_dense_matching_amd import randla
    torch.manual_seed(d_out)
    blk = randla.BuildingBlock(d_out).cuda().eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.3)
    B, K = 3, 16
    xyz = torch.randn(B, n, 3, device="cuda")
    feat = torch.randn(B, d_out // 2, n, 1, device="cuda")
    idx = torch.randint(0, n, (B, n, K), device="cuda", dtype=torch.int32)
    with torch.no_grad():
        settings.USE_FUSED_LFA = False
        ref = blk(xyz, feat, idx)
        settings.USE_FUSED_LFA = True
        got = blk(xyz, feat, idx)
    assert got.shape == ref.shape == (B, d_out, n, 1)
    err = (got - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("B,N,Ca", [(2, 100, 128), (1, 2048, 64), (3, 64, 72)])
def test_point_heads_chain_equals_the_layers_in_fp64(ops, B, N, Ca):
    """The per-point heads of GeoMatch.forward as one launch (/root/reference/models/geoMatch.py:159-200: feature_encoding_layer x4,
    normalize_feature_layer, + rgbd_emb, seg_layer x4) == the same chain of 1x1 convolutions, affine maps and ReLUs in fp64.
    Ragged N (not a multiple of the 64-point workgroup), the input given whole or as two channel blocks."""
    rs = np.random.RandomState(N + Ca)
    x0 = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32))
    Ws = [torch.from_numpy((rs.randn(128, 128) / 11).astype(np.float32)) for _ in range(8)]
    sc = [torch.from_numpy((rs.rand(128) + 0.5).astype(np.float32)) for _ in range(8)]
    sh = [torch.from_numpy((rs.randn(128) * 0.3).astype(np.float32)) for _ in range(8)]
    acts = [1, 1, 1, 0, 1, 1, 1, 1]
    sc[3], sh[3] = None, None                                       # the fourth layer: no BN, no bias, no activation
    w_last = torch.from_numpy((rs.randn(2, 128) / 11).astype(np.float32))
    b_last = torch.from_numpy(rs.randn(2).astype(np.float32))
    x = x0.double()
    feat = None
    for l in range(8):
        y = torch.einsum("oc,bcn->bon", Ws[l].double(), x)
        if sc[l] is not None:
            y = y * sc[l].double()[None, :, None] + sh[l].double()[None, :, None]
        if l == 3:
            feat = y
        if acts[l]:
            y = y.clamp(min=0)
        if l == 4:
            y = x0.double() + y
        x = y
    seg = torch.einsum("oc,bcn->bon", w_last.double(), x) + b_last.double()[None, :, None]
    layers = [(ops.gemm_pack_weight(Ws[l].cuda()), sc[l].cuda() if sc[l] is not None else None,
               sh[l].cuda() if sh[l] is not None else None, acts[l]) for l in range(8)]
    last = (ops.gemm_pack_weight(w_last.cuda()), b_last.cuda(), 2)
    a = x0[:, :Ca].contiguous().cuda()
    bq = x0[:, Ca:].contiguous().cuda() if Ca < 128 else None
    got_feat, got_seg = ops.point_heads(a, bq, layers, last, feat_layer=3, res_layer=4)
    assert got_feat.shape == (B, 128, N) and got_seg.shape == (B, 2, N)
    assert (got_feat.cpu().double() - feat).abs().max().item() < 3e-5 * max(1.0, feat.abs().max().item())
    assert (got_seg.cpu().double() - seg).abs().max().item() < 5e-5 * max(1.0, seg.abs().max().item())


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 64, 128, 64, 64), (1, 128, 256, 16, 64), (3, 256, 64, 8, 128)])
def test_strided_conv3x3_and_conv1x1_downsample_vs_fp64(ops, B, Cin, Cout, H, W):
    """Stride-2 forms of the implicit-GEMM kernel (first block of ResNet-18 layer2, /root/reference/models/cnn/extractors.py:151-177):
    3x3 / pad 1 / stride 2 with BN + ReLU in the epilogue, fp32 and packed outputs, and the 1x1 / stride 2 downsample branch on the
    same packed input == F.conv2d in fp64."""
    rs = np.random.RandomState(Cin + W)
    x = torch.from_numpy(rs.randn(B, Cin, H, W).astype(np.float32))
    w3 = torch.from_numpy((rs.randn(Cout, Cin, 3, 3) / np.sqrt(9 * Cin)).astype(np.float32))
    w1 = torch.from_numpy((rs.randn(Cout, Cin) / np.sqrt(Cin)).astype(np.float32))
    scale = torch.from_numpy((rs.rand(Cout) + 0.5).astype(np.float32))
    shift = torch.from_numpy(rs.randn(Cout).astype(np.float32))
    ref3 = torch.nn.functional.conv2d(x.double(), w3.double(), stride=2, padding=1) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    ref3 = ref3.clamp(min=0)
    ref1 = torch.nn.functional.conv2d(x.double(), w1.double()[:, :, None, None], stride=2) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    assert ops.conv3x3_supported(x.cuda(), w3.cuda(), (2, 2))
    xp = ops.conv3x3_pack_act(x.cuda())
    got = ops.conv3x3_bf16x3(xp, ops.conv3x3_pack_weight(w3.cuda()), Cout, scale.cuda(), shift.cuda(), ops.ACT_RELU, stride=2)
    assert got.shape == (B, Cout, H // 2, W // 2)
    tol = 3e-5 * max(1.0, ref3.abs().max().item())
    assert (got.cpu().double() - ref3).abs().max().item() < tol
    if (B * (H // 2) * (W // 2)) % 256 == 0:
        # packed output of the strided convolution feeds a stride-1 convolution (conv1 -> conv2 of the block)
        _, opk = ops.conv3x3_bf16x3(xp, ops.conv3x3_pack_weight(w3.cuda()), Cout, scale.cuda(), shift.cuda(), ops.ACT_RELU, out_f32=False,
                                    out_packed=True, stride=2)
        if Cout == 64 or Cout % 128 == 0:
            w2 = torch.from_numpy((rs.randn(64, Cout, 3, 3) / np.sqrt(9 * Cout)).astype(np.float32))
            ref2 = torch.nn.functional.conv2d(ref3, w2.double(), padding=1)
            got2 = ops.conv3x3_bf16x3(opk, ops.conv3x3_pack_weight(w2.cuda()), 64)
            assert (got2.cpu().double() - ref2).abs().max().item() < 5e-5 * max(1.0, ref2.abs().max().item())
    got1 = ops.conv1x1_packed2d(xp, ops.gemm_pack_weight(w1.cuda()), Cout, scale.cuda(), shift.cuda(), ops.ACT_NONE, stride=2)
    assert (got1.cpu().double() - ref1).abs().max().item() < 3e-5 * max(1.0, ref1.abs().max().item())
    got1s = ops.conv1x1_packed2d(xp, ops.gemm_pack_weight(w1.cuda()), Cout, None, None, ops.ACT_NONE, stride=1)
    ref1s = torch.nn.functional.conv2d(x.double(), w1.double()[:, :, None, None])
    assert (got1s.cpu().double() - ref1s).abs().max().item() < 3e-5 * max(1.0, ref1s.abs().max().item())


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 128, 128), (1, 3, 7, 9), (2, 5, 16, 6)])
def test_affine_relu_maxpool_equals_modules(ops, B, C, H, W):
    """BN (folded) + ReLU + MaxPool2d(3, 2, 1) in one pass == the three modules (stem of /root/reference/models/cnn/extractors.py:128-131);
    odd sizes exercise the pool's padding at both ends.  Selection + one fma: exact against the same fp32 arithmetic."""
    rs = np.random.RandomState(H * W)
    x = torch.from_numpy(rs.randn(B, C, H, W).astype(np.float32)).cuda()
    scale = torch.from_numpy((rs.rand(C) + 0.5).astype(np.float32)).cuda()
    shift = torch.from_numpy(rs.randn(C).astype(np.float32)).cuda()
    ref = torch.nn.functional.max_pool2d(torch.relu(torch.addcmul(shift[None, :, None, None], x, scale[None, :, None, None])), 3, 2, 1)
    got = ops.affine_relu_maxpool(x, scale, shift)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("B,n,cs,cout,n_src,pm", [
    (16, 2048, (8,), 16, None, False),                # DilatedResBlock(8, 32).mlp1
    (16, 2048, (32, 8), 64, None, False),             # its tail lrelu(bn(mlp2(f)) + bn(shortcut(x))) as one layer over [f ; x]
    (16, 8, (512, 512), 512, None, False),            # deepest r2p fuse over cat(p_emb0, r2p_emb): 8 points per crop, K split in 4
    (16, 8, (512,), 1024, None, False),               # deepest p2r pre layer: 128 points, 1024 channels out
    (16, 32, (256, 256), 512, None, False),           # level-3 tail: K split in 2
    (2, 512, (64, 128), 64, 128, False),              # decoder over cat(skip, nearest_interpolation(deeper))
    (3, 37, (5, 3, 6), 7, 11, False),                 # ragged everything, three segments
    (1, 50, (70,), 3, None, False),                   # ragged K with the split (few points)
    (2, 36, (512,), 1024, None, False),               # PSP prior at 6 x 6: n % 4 == 0 with a PARTIAL last tile (72 points): the
    (1, 4, (64, 64), 48, None, False),                #   16-byte operand loads of the out-of-range lanes must stay inside the array
    (4, 512, (64,), 64, None, True),                  # point-major product for the 64-channel fusion kernel
    (2, 130, (70,), 130, None, True),
    (8, 16384, (32,), 64, None, False),               # training-size layers: no K split, the four waves = four channel groups of a tile
    (8, 16384, (32,), 32, None, False),               # ... two of the four waves have channels
    (4, 32770, (40,), 72, None, False),               # ... ragged: n % 4 != 0, the second 64-channel group holds 8 valid channels
    (2, 65536, (16, 16), 80, 4096, False),            # ... an indexed segment, 80 = 64 + 16 channels
])
def test_pointwise_layer_vs_torch(ops, B, n, cs, cout, n_src, pm):
    """ops.pointwise (gdm_pointwise2_hip) == cat -> 1x1 conv -> affine (folded BN) -> activation in fp64 torch, to fp32 rounding
    of a K-term dot product (1e-5 relative to the output scale); an indexed segment = nearest interpolation of its source."""
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + n)
    xs, segs = [], []
    for j, c in enumerate(cs):
        if j == 1 and n_src is not None:
            src = torch.randn(B, c, n_src, generator=g).cuda()
            idx = torch.randint(0, n_src, (B, n, 1), generator=g).int().cuda()
            xs.append(torch.gather(src, 2, idx.view(B, 1, n).expand(B, c, n).long()))
            segs.append((src, idx))
        else:
            x = torch.randn(B, c, n, generator=g).cuda()
            xs.append(x)
            segs.append(x.unsqueeze(3) if j == 0 else x)
    K = sum(cs)
    w = (torch.randn(cout, K, generator=g) / K ** 0.5).cuda()
    scale, shift = (torch.rand(cout, generator=g) + 0.5).cuda(), torch.randn(cout, generator=g).cuda()
    want = torch.einsum("ok,bkn->bon", w.double(), torch.cat(xs, 1).double()) * scale.double().view(1, -1, 1) + shift.double().view(1, -1, 1)
    want = torch.where(want > 0, want, want * 0.2)
    got = ops.pointwise(segs, w.t().contiguous(), scale, shift, ops.ACT_LEAKY, 0.2, point_major=pm)
    if pm:
        assert got.shape == (B, n, cout)
        got = got.transpose(1, 2)
    tol = 1e-5 * max(1.0, want.abs().max().item())
    assert (got.double() - want).abs().max().item() < tol
    # channel-offset output: the layer writes channels [c0, c0 + cout) of a wider tensor and nothing else
    if not pm:
        wide = torch.full((B, cout + 9, n), 7.0, device="cuda")
        ops.pointwise(segs, w.t().contiguous(), scale, shift, ops.ACT_LEAKY, 0.2, out=wide, out_c0=5)
        assert torch.equal(wide[:, 5:5 + cout], got) and bool((wide[:, :5] == 7).all()) and bool((wide[:, 5 + cout:] == 7).all())
    # no scale / shift / activation: the plain product
    plain = ops.pointwise(segs, w.t().contiguous(), point_major=pm)
    want = torch.einsum("ok,bkn->bon", w.double(), torch.cat(xs, 1).double())
    assert ((plain.transpose(1, 2) if pm else plain).double() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("B,n,K,cout", [(8, 16384, 32, 64), (4, 4096, 64, 128), (24, 64, 256, 512), (2, 1000, 9, 8), (3, 4098, 128, 64)])
def test_pointwise_rowmajor_weight_equals_transposed_copy(ops, B, n, K, cout):
    """w_rowmajor=True reads the weight as nn.Conv holds it ([Cout, K], the training path) -- the same sums in the same order as the
    [K, Cout] copy on the MFMA form (K >= 32: bit-identical); the FMA form to fp32 rounding."""
    g = torch.Generator(device="cpu").manual_seed(n + K)
    x = torch.randn(B, K, n, generator=g).cuda()
    w = (torch.randn(cout, K, generator=g) / K ** 0.5).cuda()
    a = ops.pointwise([x], w, w_rowmajor=True)
    b = ops.pointwise([x], w.t().contiguous())
    if K >= 32:
        assert torch.equal(a, b)
    else:
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item())
    want = torch.einsum("ok,bkn->bon", w.double(), x.double())
    assert (a.double() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())


def test_dilated_res_block_tail_as_one_layer_equals_modules():
    """lrelu(bn(mlp2(f)) + bn(shortcut(x))) (RandLANet.py:685-688) through the folded two-segment layer == the torch modules (fp64)."""
    from geometric_aware_dense_matching_amd import ops as o
    from geometric_aware_dense_matching_amd.randla import DilatedResBlock
    torch.manual_seed(5)
    blk = DilatedResBlock(8, 32).cuda().eval()
    for m in (blk.mlp2, blk.shortcut):
        bn = m.bn.bn
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0); bn.weight.data.normal_(); bn.bias.data.normal_()
    f = torch.randn(3, 32, 200, 1, device="cuda")
    x = torch.randn(3, 8, 200, 1, device="cuda")
    with torch.no_grad():
        got = blk.mlp2.forward_segs([f], res=(blk.shortcut, x), act=(o.ACT_LEAKY, 0.2))
        blk64 = DilatedResBlock(8, 32).cuda().double().eval()
        blk64.load_state_dict({k: v.double() for k, v in blk.state_dict().items()})
        want = torch.nn.functional.leaky_relu(torch.nn.Sequential.forward(blk64.mlp2, f.double())
                                              + torch.nn.Sequential.forward(blk64.shortcut, x.double()), 0.2)
    assert (got.double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())


def test_pointwise_rejects_bad_arguments(ops):
    x = torch.randn(2, 8, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.pointwise([x], torch.randn(9, 4, device="cuda"))                     # weight rows != channels
    with pytest.raises(ValueError):
        ops.pointwise([x, torch.randn(2, 8, 32, device="cuda")], torch.randn(16, 4, device="cuda"))   # segments disagree on n
    with pytest.raises(RuntimeError):
        ops.pointwise([x.cpu()], torch.randn(8, 4))                              # no CPU path


@pytest.mark.parametrize("B,K,Cout,ns", [(16, 512, 1024, (1, 4, 9, 36)), (32, 512, 1024, (1, 4, 9, 36)), (2, 512, 1024, (1, 4, 9, 36)), (3, 64, 40, (5, 64)), (1, 128, 16, (7,))])
def test_pointwise_jobs_equal_separate_launches_bit_for_bit(ops, B, K, Cout, ns):
    """gdm_pointwise_jobs_hip (the four prior products of the pyramid-pooling module, pspnet.py:17-31, in one launch) == one
    gdm_pointwise2_hip launch per job, bit for bit (same tile function, same K split), and == the fp64 product at fp32 accuracy."""
    g = torch.Generator(device="cpu").manual_seed(K + Cout + len(ns))
    xs = [torch.randn(B, K, n, generator=g).cuda() for n in ns]
    wts = [(torch.randn(K, Cout, generator=g) / K ** 0.5).cuda() for _ in ns]
    got = ops.pointwise_jobs(xs, wts)
    for x, wt, y in zip(xs, wts, got):
        assert torch.equal(y, ops.pointwise([x], wt))
        want = torch.einsum("kc,bkn->bcn", wt.double(), x.double())
        assert (y.double() - want).abs().max().item() < 2e-6 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("prec", ["MATCH_BF16X3", "MATCH_F32"])
@pytest.mark.parametrize("R1,n1,n2", [(16, 2048, 8192), (3, 100, 37), (1, 4096, 64)])
def test_match_pack2_equals_two_pack_launches(ops, prec, R1, n1, n2):
    """gdm_match_pack2_hip (scene + model descriptor rows of one step in one launch, evaluator.py:80-81) writes the bytes of two
    gdm_match_pack_hip launches."""
    g = torch.Generator(device="cpu").manual_seed(R1 * 7 + n2)
    a, b = torch.randn(R1, 128, n1, generator=g).cuda(), torch.randn(128, n2, generator=g).cuda()
    p = getattr(ops, prec)
    o1, o2 = ops.match_pack2(a, b, p)
    assert torch.equal(o1, ops.match_pack(a, p)) and torch.equal(o2, ops.match_pack(b, p))


@pytest.mark.parametrize("B,n,C0,C1,C2,acts", [(16, 2048, 9, 8, 16, (2, 2)), (3, 77, 16, 16, 32, (1, 0)), (1, 5, 1, 3, 2, (0, 2))])
def test_pointwise_chain2_equals_two_launches_bit_for_bit(ops, B, n, C0, C1, C2, acts):
    """gdm_pointwise_chain2_hip (RandLA stem fc0 + the first block's mlp1, RandLANet.py:19,683) == two gdm_pointwise2_hip launches."""
    g = torch.Generator(device="cpu").manual_seed(B + n + C2)
    x = torch.randn(B, C0, n, generator=g).cuda()
    mk = lambda k, c: ((torch.randn(k, c, generator=g) / k ** 0.5).cuda(), (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda())
    (w0, s0, b0), (w1, s1, b1) = mk(C0, C1), mk(C1, C2)
    y0, y1 = ops.pointwise_chain2(x, (w0, s0, b0, acts[0], 0.2), (w1, s1, b1, acts[1], 0.2))
    r0 = ops.pointwise([x], w0, s0, b0, acts[0], 0.2)
    r1 = ops.pointwise([r0], w1, s1, b1, acts[1], 0.2)
    assert torch.equal(y0, r0) and torch.equal(y1, r1)
    y0n, y1n = ops.pointwise_chain2(x, (w0, None, None, 0, 0.0), (w1, None, b1, 1, 0.0))          # no scale / shift
    r0n = ops.pointwise([x], w0)
    assert torch.equal(y0n, r0n) and torch.equal(y1n, ops.pointwise([r0n], w1, None, b1, 1, 0.0))


def test_pointwise_jobs_mixed_k_splits_and_bad_shapes(ops):
    x = torch.randn(2, 64, 8, device="cuda")
    with pytest.raises(ValueError):
        ops.pointwise_jobs([x, torch.randn(2, 32, 8, device="cuda")], [torch.randn(64, 16, device="cuda"), torch.randn(32, 16, device="cuda")])
    big = torch.randn(4, 512, 16384, device="cuda")                              # alone: no K split; the 4-point job alone: eight parts
    small = torch.randn(4, 512, 1, device="cuda")
    w = torch.randn(512, 64, device="cuda")
    ys = ops.pointwise_jobs([small, big], [w, w])                                # two launches (one per split), still bit-identical
    assert torch.equal(ys[0], ops.pointwise([small], w)) and torch.equal(ys[1], ops.pointwise([big], w))


@pytest.mark.parametrize("B,H,W", [(2, 256, 256), (1, 100, 70), (3, 64, 128), (1, 7, 9)])
def test_stem_kernel_vs_torch_fp64(ops, B, H, W):
    """gdm_stem_hip == maxpool3x3/2/p1(relu(bn(conv7x7/2/p3(x)))) (extractors.py:112-116,181-185) in fp64 torch: split-bf16 products
    (|err| <= 3 * 2^-16 |w x| per product -- |lo| <= 2^-8 |v|, residual <= 2^-16 |v| -- over 147 terms): 2e-5 relative to the output scale.  The packed operand it also writes is
    byte-identical to what the pack kernel makes of its fp32 output."""
    from geometric_aware_dense_matching_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(H * 7 + W)
    x = torch.randn(B, 3, H, W, generator=g).cuda()
    w = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).cuda()
    scale, shift = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.3).cuda()
    got = ops.stem(x, ops.stem_pack_weight(w), scale, shift)
    y = torch.nn.functional.conv2d(x.double(), w.double(), stride=2, padding=3)
    y = torch.relu(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    want = torch.nn.functional.max_pool2d(y, 3, 2, 1)
    assert got.shape == want.shape
    assert (got.double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())
    pk = getattr(got, "_gdm_packed", None)
    PH, PW = got.shape[2], got.shape[3]
    if (B * PH * PW) % 256 == 0 and PW % 16 == 0:
        assert pk is not None and pk.shape == tuple(got.shape)
        mine = pk.buf.clone()                                     # the pool may hand the same buffer to the pack launch below
        ref = ops.conv3x3_pack_act(got.clone())
        assert torch.equal(ref.buf, mine)
    else:
        assert pk is None


@pytest.mark.parametrize("B,C,H,W", [(16, 1024, 32, 32), (2, 128, 32, 32), (1, 64, 16, 32), (3, 24, 10, 12)])
def test_psp_combine_with_packed_output(ops, B, C, H, W):
    """psp_combine (pspnet.py:24-31 without the 2560-channel concat): the eight-planes-per-workgroup form that also writes the packed
    operand == the one-plane form bit for bit (same expression, same order), == relu(g + bias + sum of align_corners interpolations)
    in fp64; its packed operand is byte-identical to what the pack kernel makes of the fp32 result."""
    g0 = torch.Generator(device="cpu").manual_seed(C + H)
    g = torch.randn(B, C, H, W, generator=g0).cuda()
    ys = [torch.randn(B, C, s, s, generator=g0).cuda() for s in (1, 2, 3, 6)]
    bias = torch.randn(C, generator=g0).cuda()
    plain = ops.psp_combine(g.clone(), ys, bias)
    assert getattr(plain, "_gdm_packed", None) is None
    want = g.double() + bias.double().view(1, -1, 1, 1)
    for y in ys:
        want = want + torch.nn.functional.interpolate(y.double(), size=(H, W), mode="bilinear", align_corners=True)
    want = torch.relu(want)
    assert (plain.double() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())
    got = ops.psp_combine(g.clone(), ys, bias, packed=True)
    assert torch.equal(got, plain)
    pk = getattr(got, "_gdm_packed", None)
    if (C == 64 or C % 128 == 0) and W % 32 == 0 and (B * H * W) % 256 == 0:
        assert pk is not None and pk.shape == (B, C, H, W)
        mine = pk.buf.clone()
        assert torch.equal(ops.conv3x3_pack_act(got.clone()).buf, mine)
    else:
        assert pk is None


@pytest.mark.parametrize("B,C,H,W,act", [(16, 256, 32, 32, 2), (2, 128, 16, 16, 1), (1, 64, 16, 32, 0)])
def test_upconv_gather_eight_channel_form_with_packed_output(ops, B, C, H, W, act):
    """upconv3x3_gather (the 9-tap bilinear gather that completes conv3x3(upsample x2) + BN + activation, pspnet.py:34-45): the
    eight-channels-per-workgroup form == the one-channel form bit for bit, and its packed operand is byte-identical to what the pack
    kernel makes of the fp32 result."""
    g0 = torch.Generator(device="cpu").manual_seed(C + H + act)
    z = torch.randn(B, 9 * C, H, W, generator=g0).cuda()
    scale, shift = (torch.rand(C, generator=g0) + 0.5).cuda(), (torch.randn(C, generator=g0) * 0.3).cuda()
    plain = ops.upconv3x3_gather(z, scale, shift, C, (2 * H, 2 * W), act, 0.25)
    got = ops.upconv3x3_gather(z, scale, shift, C, (2 * H, 2 * W), act, 0.25, packed=True)
    assert getattr(plain, "_gdm_packed", None) is None
    assert torch.equal(got, plain)
    pk = getattr(got, "_gdm_packed", None)
    if (2 * W) % 32 == 0 and (B * 4 * H * W) % 256 == 0:
        assert pk is not None and pk.shape == (B, C, 2 * H, 2 * W)
        mine = pk.buf.clone()
        assert torch.equal(ops.conv3x3_pack_act(got.clone()).buf, mine)
    else:
        assert pk is None


@pytest.mark.parametrize("B,H,W,n,act", [(16, 64, 64, 512, 1), (2, 8, 32, 100, 2)])
def test_conv64_fusion_kernel_packed_output(ops, B, H, W, n, act):
    """conv64_gather_add_act_mfma with hw: same fp32 result as without, and a packed operand byte-identical to the pack kernel's."""
    g0 = torch.Generator(device="cpu").manual_seed(H + n)
    m = H * W
    x = torch.randn(B, 64, m, generator=g0).cuda()
    wpk = ops.pack_rows64((torch.randn(64, 64, generator=g0) / 8).cuda())
    t = torch.randn(B, n, 64, generator=g0).cuda()
    idx = torch.randint(0, n, (B, m), generator=g0, dtype=torch.int32).cuda()
    scale, shift = (torch.rand(64, generator=g0) + 0.5).cuda(), (torch.randn(64, generator=g0) * 0.3).cuda()
    plain = ops.conv64_gather_add_act_mfma(x, wpk, t, idx, scale, shift, act, 0.2, t_point_major=True)
    got = ops.conv64_gather_add_act_mfma(x, wpk, t, idx, scale, shift, act, 0.2, t_point_major=True, hw=(H, W))
    assert torch.equal(got, plain)
    pk = getattr(got, "_gdm_packed", None)
    assert pk is not None and pk.shape == (B, 64, H, W)
    mine = pk.buf.clone()
    assert torch.equal(ops.conv3x3_pack_act(got.view(B, 64, H, W).clone()).buf, mine)


def test_point_heads_in_two_launches_equals_one(ops):
    """The heads chain as GeoMatch.forward(defer_seg=True) launches it -- four feature layers, then normalise + residual + segmentation
    layers with the embedding as the residual source -- == the one-launch chain, bit for bit."""
    rs = np.random.RandomState(7)
    B, N = 3, 300
    x0 = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32)).cuda()
    a, b = x0[:, :64].contiguous(), x0[:, 64:].contiguous()
    layers = [(ops.gemm_pack_weight(torch.from_numpy((rs.randn(128, 128) / 11).astype(np.float32)).cuda()),
               None if l == 3 else torch.from_numpy((rs.rand(128) + 0.5).astype(np.float32)).cuda(),
               None if l == 3 else torch.from_numpy((rs.randn(128) * 0.3).astype(np.float32)).cuda(), 0 if l == 3 else 1) for l in range(8)]
    last = (ops.gemm_pack_weight(torch.from_numpy((rs.randn(2, 128) / 11).astype(np.float32)).cuda()),
            torch.from_numpy(rs.randn(2).astype(np.float32)).cuda(), 2)
    feat1, seg1 = ops.point_heads(a, b, layers, last, 3, 4)
    feat2, none = ops.point_heads(a, b, layers[:4], None, 3, -1)
    assert none is None
    none2, seg2 = ops.point_heads(feat2, None, layers[4:], last, -1, 0, residual=(a, b))
    assert none2 is None
    assert torch.equal(feat1, feat2) and torch.equal(seg1, seg2)


def test_call_helper_reads_the_stream_at_call_time(ops):
    """ops.match_score (one kernel, through _lib.call) captured under torch.cuda.graph and replayed == the eager result.  Capture
    runs on a stream of its own: a helper that had read the stream earlier would launch outside the capture, which raises."""
    rs = np.random.RandomState(11)
    B, N = 2, 70
    conf = torch.from_numpy(rs.rand(B, N).astype(np.float32)).cuda()
    mask = torch.from_numpy((rs.rand(B, N) < 0.6).astype(np.uint8)).cuda()
    eager = ops.match_score(conf, mask)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.match_score(conf, mask)
    out.zero_()                                     # what capture left in the buffer is not the result
    g.replay()
    torch.cuda.synchronize()
    assert float(eager.abs().min()) > 0 and torch.equal(out, eager)
