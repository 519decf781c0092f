"""GPU: the fused inference path of the DGCNN variant (geoMatch_DGCNN.GeoMatch, BASELINE config 4).

  ops.feature_knn   k nearest neighbours in feature space, Gram tile and selection in one kernel (no [B,n,n] matrix), against
                    oracle.dgcnn_ref.knn on the CPU: graphs equal except at fp32 near-ties, values against the fp64 score
  ops.edge_block    one edge-convolution stage without the [B,2C,n,k] edge tensor, against an fp64 restatement of
                    get_graph_feature -> conv -> eval BN -> LeakyReLU [-> conv -> BN -> LeakyReLU] -> max over k
  the model         `fused=True` against the reference-made golden and against the oracle with its graphs injected; as a pipeline step
                    and a hipGraph; without a dense [M,M] allocation at M = 16384
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from geometric_aware_dense_matching_amd import synthetic  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _knn_input(kind, B, C, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, n, generator=g)
    if kind == "xyz":                                   # a crop 0.9 m from the camera, 5 cm across: xx ~ 0.81, distances ~ 1e-3
        return 0.05 * x + torch.tensor([0.0, 0.0, 0.9]).view(1, 3, 1)
    if kind == "lrelu":                                 # what the second and third graphs see: activations
        return torch.nn.functional.leaky_relu(x, 0.2)
    if kind == "cluster":                               # every 16th point in one tight cluster: a row's whole neighbourhood sits in ONE
        x = 3.0 * x                                     # column class modulo 16, which overflows the kernel's short private lists
        x[:, :, ::16] = 0.1 * torch.randn(B, C, (n + 15) // 16, generator=g)          # (around the origin: no cancellation in the scores)
        return x
    assert kind == "randn"
    return x


def _score64(x):
    """dgcnn.py:22-25 in fp64: s[b,r,c] = -xx[c] + 2 g[r,c] - xx[r]; and max xx of the fp32 input."""
    xd = x.double()
    xx = (xd ** 2).sum(dim=1, keepdim=True)
    return -xx + 2 * torch.matmul(xd.transpose(2, 1), xd) - xx.transpose(2, 1), float(xx.max())


def _check_graph(idx, want_idx, dist):
    from oracle import dgcnn_ref
    same = (torch.sort(idx, -1)[0] == torch.sort(want_idx, -1)[0]).all(dim=-1).float().mean().item()
    bad = dgcnn_ref.graph_mismatch_not_near_tie(idx, want_idx, dist, tol=2e-4)
    print("rows with the oracle's neighbour set: %.5f, mismatches that are no near-tie: %d" % (same, bad))
    assert same >= 0.995
    assert bad == 0


# (B, C, n, k, input kind, seed).  The first six are the shapes the trunks meet in small: both k, the xyz graph's cancellation,
# several ragged column tiles, fewer columns than two tiles, two channel chunks.  Then: the exact redo with both forms of its bound
# (cluster, k = 16 and k = 20), a partial second channel chunk, and k <= 8 (lists as long as k: no redo pass).
KNN_CASES = [(2, 64, 1000, 16, "randn", 101), (1, 64, 1000, 20, "randn", 102), (2, 3, 1000, 16, "xyz", 103),
             (1, 64, 2500, 20, "lrelu", 104), (2, 64, 67, 16, "randn", 105), (1, 128, 700, 20, "lrelu", 106),
             (1, 64, 1024, 16, "cluster", 107), (1, 70, 300, 16, "randn", 108), (1, 64, 200, 8, "randn", 109),
             (1, 64, 1024, 20, "cluster", 112)]


@pytest.mark.parametrize("B,C,n,k,kind,seed", KNN_CASES)
def test_feature_knn_vs_oracle(B, C, n, k, kind, seed):
    from geometric_aware_dense_matching_amd import ops
    from oracle import dgcnn_ref
    x = _knn_input(kind, B, C, n, seed)
    want_idx, dist = dgcnn_ref.knn(x, k)
    idx, val = ops.feature_knn(x.cuda(), k, return_values=True)
    assert idx.shape == (B, n, k) and idx.dtype == torch.int32 and val.shape == (B, n, k)
    idx, val = idx.long().cpu(), val.cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    _check_graph(idx, want_idx, dist)
    assert torch.equal(ops.feature_knn(x.cuda(), k).long().cpu(), idx)                  # without values: the same graph
    # values: non-increasing along k, equal values in ascending column order, and the fp64 score of the chosen column to the rounding
    # of C fp32 products and sums on magnitudes up to 4 max xx
    assert bool((val[..., 1:] <= val[..., :-1]).all())
    tie = val[..., 1:] == val[..., :-1]
    assert bool((idx[..., 1:][tie] > idx[..., :-1][tie]).all())
    s64, xxmax = _score64(x)
    err = (val.double() - s64.gather(2, idx)).abs().max().item()
    bound = (C + 4) * 2.0 ** -22 * xxmax
    print("max |val - s64[idx]| = %.3e, bound %.3e" % (err, bound))
    assert err <= bound


@pytest.mark.parametrize("B,C,n,k,kind,seed", [(2, 64, 1000, 16, "randn", 101), (1, 64, 1024, 20, "cluster", 112), (1, 128, 333, 20, "lrelu", 113)])
def test_feature_knn_does_not_depend_on_the_column_split(B, C, n, k, kind, seed):
    """1, 2 or 4 waves per row group (the launcher picks by the number of workgroups; small shapes always get 4): same bits."""
    from geometric_aware_dense_matching_amd import ops
    from oracle import dgcnn_ref
    x = _knn_input(kind, B, C, n, seed)
    want_idx, dist = dgcnn_ref.knn(x, k)
    ref = ops.feature_knn(x.cuda(), k, return_values=True)
    for splits in (1, 2, 4):
        got = ops.feature_knn(x.cuda(), k, return_values=True, splits=splits)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), splits
    _check_graph(ref[0].long().cpu(), want_idx, dist)


def test_feature_knn_reads_a_channel_slice_in_place():
    """The xyz graph of the first stage is built from channels 0..2 of the 9-channel input: the batch stride is passed on, no copy."""
    from geometric_aware_dense_matching_amd import ops
    g = torch.Generator().manual_seed(110)
    x9 = torch.randn(2, 9, 333, generator=g).cuda()
    x9[:, :3] = 0.05 * x9[:, :3] + torch.tensor([0.0, 0.0, 0.9], device="cuda").view(1, 3, 1)
    assert torch.equal(ops.feature_knn(x9[:, :3], 16), ops.feature_knn(x9[:, :3].contiguous(), 16))


def test_feature_knn_ties_and_short_rows():
    from geometric_aware_dense_matching_amd import ops
    g = torch.Generator().manual_seed(111)
    x = torch.randn(2, 64, 256, generator=g)
    x[:, :, 128:] = x[:, :, :128]                       # every point twice: identical columns, identical scores -> the tie rule decides
    idx = ops.feature_knn(x.cuda(), 16).long().cpu()
    r = torch.arange(256) % 128
    assert torch.equal(idx[:, :, 0], r.expand(2, 256)) and torch.equal(idx[:, :, 1], (r + 128).expand(2, 256))
    x = torch.randn(1, 64, 10, generator=g)
    idx = ops.feature_knn(x.cuda(), 16).long().cpu()
    assert torch.equal(torch.sort(idx[0, :, :10], dim=-1)[0], torch.arange(10).expand(10, 10))
    assert bool((idx[0, :, 10:] == 0).all())


def _bn_params(g, c=64):
    w = torch.randn(c, generator=g).double()            # both signs
    w = torch.where(w.abs() < 0.2, torch.full_like(w, 0.5), w)
    return dict(weight=w, bias=0.3 * torch.randn(c, generator=g).double(), mean=0.2 * torch.randn(c, generator=g).double(),
                var=(0.5 + torch.rand(c, generator=g)).double())


def _bn64(y, p):
    sh = [1, -1] + [1] * (y.dim() - 2)
    return (y - p["mean"].view(sh)) / torch.sqrt(p["var"].view(sh) + 1e-5) * p["weight"].view(sh) + p["bias"].view(sh)


def _fold32(p):
    scale = p["weight"] / torch.sqrt(p["var"] + 1e-5)
    return scale.float().cuda(), (p["bias"] - p["mean"] * scale).float().cuda()


# (B, C, n, k, two convolutions, channel slice of the [B,192,n] buffer, seed)
EDGE_CASES = [(2, 9, 200, 16, True, 0, 121), (1, 64, 333, 20, True, 64, 122), (2, 64, 200, 16, False, 128, 123)]


@pytest.mark.parametrize("B,C,n,k,two,c0,seed", EDGE_CASES)
def test_edge_block_vs_fp64_restatement(B, C, n, k, two, c0, seed):
    from geometric_aware_dense_matching_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, n, generator=g)
    idx = torch.randint(0, n, (B, n, k), generator=g)
    idx[:, :, 0] = torch.arange(n)                      # self-loops
    idx[:, :, 3] = idx[:, :, 2]                         # a repeated neighbour
    w1 = torch.randn(64, 2 * C, generator=g) / (2 * C) ** 0.5
    w2 = torch.randn(64, 64, generator=g) / 8.0
    bn1, bn2 = _bn_params(g), _bn_params(g)
    # dgcnn.py:30-56 get_graph_feature -> conv -> eval BN -> LeakyReLU(0.2) [-> conv -> BN -> LeakyReLU] -> max over k, in fp64
    xd = x.double()
    xj = torch.gather(xd.unsqueeze(2).expand(B, C, n, n), 3, idx.unsqueeze(1).expand(B, C, n, k))       # [B,C,n,k]
    xi = xd.unsqueeze(3).expand(B, C, n, k)
    y = torch.einsum("oc,bcnk->bonk", w1.double(), torch.cat((xj - xi, xi), dim=1))
    y = torch.nn.functional.leaky_relu(_bn64(y, bn1), 0.2)
    if two:
        y = torch.nn.functional.leaky_relu(_bn64(torch.einsum("oc,bcnk->bonk", w2.double(), y), bn2), 0.2)
    want = y.max(dim=-1)[0]
    # the product: the split first convolution per point, then the edge kernel into a slice of a NaN-filled [B,192,n] buffer
    wt = torch.cat((w1[:, :C], w1[:, C:] - w1[:, :C]), dim=0).t().contiguous().cuda()
    pq = ops.pointwise([x.cuda()], wt, point_major=True)
    assert pq.shape == (B, n, 128)
    buf = torch.full((B, 192, n), float("nan"), device="cuda")
    s1, t1 = _fold32(bn1)
    s2, t2 = _fold32(bn2)
    out = ops.edge_block(pq, idx.cuda(), s1, t1, *((w2.cuda(), s2, t2) if two else (None, None, None)), slope=0.2, out=buf, out_c0=c0)
    assert out is buf
    got = buf[:, c0:c0 + 64].cpu().double()
    err = (got - want).abs().max().item()
    print("max |got - want| = %.3e, bound %.3e" % (err, 5e-4 * max(1.0, want.abs().max().item())))
    assert err < 5e-4 * max(1.0, want.abs().max().item())
    rest = torch.cat((buf[:, :c0], buf[:, c0 + 64:]), dim=1)
    assert bool(torch.isnan(rest).all())
    # without `out`: the same values in a tensor of its own; an index outside [0, n) is clamped, not followed
    bad = idx.clone()
    bad[:, :, 1] = torch.where(torch.arange(n) % 2 == 0, torch.tensor(-5), torch.tensor(n + 7))
    alone = ops.edge_block(pq, idx.cuda(), s1, t1, *((w2.cuda(), s2, t2) if two else (None, None, None)))
    assert torch.equal(alone, buf[:, c0:c0 + 64])
    clamped = ops.edge_block(pq, bad.cuda(), s1, t1, *((w2.cuda(), s2, t2) if two else (None, None, None)))
    same = ops.edge_block(pq, bad.clamp(0, n - 1).cuda(), s1, t1, *((w2.cuda(), s2, t2) if two else (None, None, None)))
    assert torch.equal(clamped, same)


def _golden_model():
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    keys = json.load(open(os.path.join(G, "dgcnn_state.json")))
    model = GeoMatchDGCNN(dict(feat_dim=128, k=16, embed_dim=1024, dropout=0.1, n_mesh_node=384), 1,
                          model_points=synthetic.make_model_points(1, 384))
    model.model_emb.k = 20
    sd = synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items() if k != "model_emb.mesh"}, seed=9)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def test_fused_model_vs_reference_golden():
    """The construction and the criteria of test_gpu_model.test_dgcnn_variant_vs_reference_golden_and_oracle, on the fused path."""
    from geometric_aware_dense_matching_amd import dgcnn
    g = np.load(os.path.join(G, "dgcnn_eval.npz"))
    model = _golden_model()
    x = torch.from_numpy(synthetic.make_batch(seed=8, batch=2, n_points=512)["cld_rgb_nrm"]).cuda()
    with torch.no_grad():
        ep = model(dict(cld_rgb_nrm=x), fused=True)
        emb = model.pcd_emb(x, fused=True)
    idx3 = dgcnn.knn_fused(x[:, :3].contiguous(), 16).cpu().numpy()
    assert (np.sort(idx3, axis=-1) == np.sort(g["knn_xyz"], axis=-1)).mean() > 0.995
    for name, t in (("emb", emb), ("rgbd", ep["rgbd"]), ("seg", ep["seg"]), ("mesh", ep["mesh"])):
        t = t.float().cpu()
        assert list(t.shape) == list(g[name + "_shape"])
        got = t.reshape(-1)[torch.from_numpy(g[name + "_pos"])].numpy()
        scale = max(1.0, float(np.abs(g[name + "_val"]).max()))
        share = (np.abs(got - g[name + "_val"]) < 5e-4 * scale).mean()
        print("%s: share within 5e-4 * scale = %.4f, norm %.6g vs %.6g" % (name, share, t.double().norm().item(), float(g[name + "_norm"])))
        assert share > 0.99, name
        assert abs(t.double().norm().item() - float(g[name + "_norm"])) < 2e-3 * float(g[name + "_norm"])


def test_fused_path_refuses_training_mode():
    model = _golden_model()
    x = torch.from_numpy(synthetic.make_batch(seed=8, batch=2, n_points=512)["cld_rgb_nrm"]).cuda()
    model.train()
    with pytest.raises(RuntimeError, match="inference only"):
        model.pcd_emb(x, fused=True)
    with pytest.raises(RuntimeError, match="inference only"):
        model.model_emb(fused=True)
    with pytest.raises(RuntimeError, match="inference only"):
        model(dict(cld_rgb_nrm=x), fused=True)


@pytest.fixture(scope="module")
def oracle_case():
    """Model, input, the oracle's outputs and its six graphs at N = 1024, M = 1536, batch 2: computed once, read only."""
    from geometric_aware_dense_matching_amd.config import make_dgcnn_cfg
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    from oracle import dgcnn_ref, model_ref
    N, M, B = 1024, 1536, 2
    torch.manual_seed(0)
    model = GeoMatchDGCNN(make_dgcnn_cfg(n_mesh_node=M, dataset="ycbv"), 2, model_points=synthetic.make_model_points(2, M, 269.573))
    sd = synthetic.synthetic_state_dict({k: v for k, v in model.state_dict().items() if k != "model_emb.mesh"}, seed=4)
    model.load_state_dict(sd, strict=False)
    model = model.cuda().eval()
    sd_cpu = {k: v.cpu() for k, v in model.state_dict().items()}
    x = torch.from_numpy(synthetic.make_batch(seed=45, batch=B, n_points=N)["cld_rgb_nrm"])
    torch.set_num_threads(16)
    with torch.no_grad():
        km = model.model_emb.k
        want = dgcnn_ref.geomatch_dgcnn_forward(sd_cpu, x, k_cloud=16, k_mesh=km)
        graphs = (dgcnn_ref.trunk_graphs(x, model_ref.SD(sd_cpu, "pcd_emb."), 16)
                  + dgcnn_ref.trunk_graphs(sd_cpu["model_emb.mesh"], model_ref.SD(sd_cpu, "model_emb."), km))
    return model, x, want, graphs, (N, M, B)


def test_fused_model_with_the_oracles_graphs_injected(oracle_case):
    from geometric_aware_dense_matching_amd import dgcnn
    model, x, want, graphs, (N, M, B) = oracle_case
    real = dgcnn.knn_fused
    queue = [g[0].to(torch.int32).cuda() for g in graphs]
    dgcnn.knn_fused = lambda feat, k: queue.pop(0)
    try:
        with torch.no_grad():
            ep = model(dict(cld_rgb_nrm=x.cuda()), fused=True)
    finally:
        dgcnn.knn_fused = real
    assert not queue
    assert ep["rgbd"].shape == (B, 128, N) and ep["mesh"].shape == (1, 128, M) and ep["seg"].shape == (B, 2, N)
    for name in ("rgbd", "seg", "mesh"):
        a, b = ep[name].cpu(), want[name]
        err, bound = (a - b).abs().max().item(), 5e-4 * max(1.0, b.abs().max().item())
        print("%s: max |got - want| = %.3e, bound %.3e" % (name, err, bound))
        assert err < bound, name


def test_fused_model_with_its_own_graphs(oracle_case):
    from geometric_aware_dense_matching_amd import dgcnn
    model, x, want, graphs, _ = oracle_case
    real = dgcnn.knn_fused
    seen = []

    def recording(feat, k):
        idx = real(feat, k)
        seen.append(idx.long().cpu())
        return idx
    dgcnn.knn_fused = recording
    try:
        with torch.no_grad():
            ep = model(dict(cld_rgb_nrm=x.cuda()), fused=True)
    finally:
        dgcnn.knn_fused = real
    assert len(seen) == 6
    for (want_idx, dist), idx in zip(graphs[:1] + graphs[3:4], seen[:1] + seen[3:4]):     # xyz graphs: same inputs on both sides
        _check_graph(idx, want_idx, dist)
    for name in ("rgbd", "seg", "mesh"):                            # free-running: feature-space graphs may flip near-ties
        a, b = ep[name].cpu().double(), want[name].double()
        print("%s: norm %.6g vs %.6g" % (name, a.norm().item(), b.norm().item()))
        assert abs(a.norm().item() - b.norm().item()) < 2e-3 * b.norm().item(), name


def _pipeline_model(M):
    from geometric_aware_dense_matching_amd.config import make_dgcnn_cfg
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    torch.manual_seed(0)
    model = GeoMatchDGCNN(make_dgcnn_cfg(n_mesh_node=M, dataset="ycbv"), 2, model_points=synthetic.make_model_points(2, M, 269.573))
    sd = synthetic.synthetic_state_dict({k: v for k, v in model.state_dict().items() if k != "model_emb.mesh"}, seed=4)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def test_pipeline_step_and_graphed_pipeline():
    from geometric_aware_dense_matching_amd import infer
    B, N, M = 2, 1024, 1024
    model = _pipeline_model(M)
    batches = [dict(cld_rgb_nrm=torch.from_numpy(synthetic.make_batch(seed=s, batch=B, n_points=N)["cld_rgb_nrm"]).cuda()) for s in (131, 132)]
    with torch.no_grad():
        eager = [infer.pipeline_step(model, b, with_pose=True) for b in batches]
    out = eager[0]
    shapes = dict(seg=(B, 2, N), rgbd=(B, 128, N), mesh=(1, 128, M), mask=(B, N), count=(B,), best_idx=(B, N), best_sim=(B, N),
                  RT=(B, 3, 4), valid=(B,))
    for name, shape in shapes.items():
        assert tuple(out[name].shape) == shape, name
    assert all(bool(torch.isfinite(out[k]).all()) for k in ("seg", "rgbd", "mesh", "best_sim"))
    gp = infer.GraphedPipeline(model, batches[0])
    print("form %s, check %r" % (gp.form, gp.check))
    assert gp.check["single"]["bit_identical"]
    assert gp.form in ("single", "forked")
    for i in (0, 1, 0, 1):
        ok, bad = infer.outputs_equal(eager[i], gp(batches[i]))
        assert ok, (i, bad)


def test_fused_forward_allocates_no_dense_matrix():
    """M = 16384: one [M,M] fp32 matrix is 1.07 GB.  The fused forward's peak stays below half of that."""
    B, N, M = 1, 1024, 16384
    model = _pipeline_model(M)
    x = torch.from_numpy(synthetic.make_batch(seed=133, batch=B, n_points=N)["cld_rgb_nrm"]).cuda()
    with torch.no_grad():
        model(dict(cld_rgb_nrm=x), fused=True)                       # warm-up: derived weights, the library
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        ep = model(dict(cld_rgb_nrm=x), fused=True)
        torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print("peak grew by %.1f MB; half an [M,M] fp32 matrix is %.1f MB" % (grew / 1e6, 0.5 * M * M * 4 / 1e6))
    assert grew < 0.5 * M * M * 4
    assert all(bool(torch.isfinite(ep[k]).all()) for k in ("rgbd", "seg", "mesh"))
