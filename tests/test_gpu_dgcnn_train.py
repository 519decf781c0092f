"""GPU: the fused TRAINING path of the DGCNN variant (geoMatch_DGCNN.GeoMatch.train_path = "fused").

  ops.edge_block_train   one edge stage with train-mode BatchNorm over all B n k edges and a full backward, against an fp64 autograd
                         restatement of get_graph_feature -> conv -> BN -> LeakyReLU [-> conv -> BN -> LeakyReLU] -> max over k;
                         without an edge tensor; under SyncBatchNorm on two gloo ranks; inside a captured graph
  the model              a whole training step against the module path with the same graphs; the train / test entry points

Measured on an MI355X, test_edge_block_train_vs_fp64_autograd, worst case over the eight (case, seed) pairs, as a fraction of each
tensor's bound (5e-4 scale for the output, 1e-4 scale for the gradients): see DESIGN.md section 6f.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from geometric_aware_dense_matching_amd import synthetic  # noqa: E402

EPS = 1e-5
SLOPE = 0.2


def _make_case(B, C, n, k, seed):
    """The inputs of one stage, drawn in a fixed order from one generator; the graph has self-loops, a repeated neighbour, a hub (7)
    that every point adds into and a point (11) that is nobody's neighbour."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, n, generator=g)
    idx = torch.randint(0, n, (B, n, k), generator=g)
    w1 = torch.randn(64, 2 * C, generator=g) / (2 * C) ** 0.5
    w2 = torch.randn(64, 64, generator=g) / 8.0
    bns = []
    for _ in range(2):
        gamma = torch.randn(64, generator=g).double()
        gamma = torch.where(gamma.abs() < 0.2, torch.full_like(gamma, 0.5), gamma)
        bns.append((gamma, 0.3 * torch.randn(64, generator=g).double()))
    idx[:, :, 0] = torch.arange(n)
    idx[:, :, 3] = idx[:, :, 2]
    idx[:, :, 5] = 7
    idx[idx == 11] = 12
    idx[:, 11, 0] = 12
    w = torch.randn(B, 64, n, generator=g).double()                        # the loss is (out * w).sum()
    run = [(0.2 * torch.randn(64, generator=g).double(), (0.5 + torch.rand(64, generator=g)).double()) for _ in range(2)]
    # the stage's first convolution per point, [W_a ; W_b - W_a] x, formed in fp64 and rounded once: the fp32 operand of the kernels
    ws = torch.cat((w1[:, :C], w1[:, C:] - w1[:, :C]), dim=0).double()
    pq = torch.einsum("oc,bcn->bno", ws, x.double()).float().contiguous()
    return dict(x=x, idx=idx, w1=w1, w2=w2, bns=bns, w=w, run=run, pq=pq, B=B, C=C, n=n, k=k)


def _bn64(gamma, beta, run):
    bn = torch.nn.BatchNorm2d(64, eps=EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(run[0]), bn.running_var.copy_(run[1])
    return bn


def _reference(case, two, lo=None, hi=None):
    """fp64 autograd on the CPU over the WHOLE batch -> dict of outputs, statistics and gradients; asserts the precondition."""
    B, C, n, k, idx = case["B"], case["C"], case["n"], case["k"], case["idx"]
    pq = case["pq"].double().requires_grad_(True)
    bi = torch.arange(B)[:, None, None]
    y1 = (pq[..., :64][bi, idx] + pq[..., 64:][:, :, None, :]).permute(0, 3, 1, 2)          # [B,64,n,k]
    # the restated first layer IS conv(get_graph_feature(x)) up to the one rounding of pq
    xd = case["x"].double()
    xj = torch.gather(xd.unsqueeze(2).expand(B, C, n, n), 3, idx.unsqueeze(1).expand(B, C, n, k))
    xi = xd.unsqueeze(3).expand(B, C, n, k)
    direct = torch.einsum("oc,bcnk->bonk", case["w1"].double(), torch.cat((xj - xi, xi), dim=1))
    assert (direct - y1.detach()).abs().max().item() < 1e-5 * max(1.0, direct.abs().max().item())
    bn1 = _bn64(*case["bns"][0], case["run"][0])
    z1 = bn1(y1)
    h = torch.nn.functional.leaky_relu(z1, SLOPE)
    pre = [z1]
    w2 = bn2 = None
    if two:
        w2 = case["w2"].double().requires_grad_(True)
        bn2 = _bn64(*case["bns"][1], case["run"][1])
        z2 = bn2(torch.einsum("oc,bcnk->bonk", w2, h))
        h = torch.nn.functional.leaky_relu(z2, SLOPE)
        pre.append(z2)
    out, arg = h.max(dim=-1)
    # precondition (a condition on the inputs, not a tolerance): no activation side and no arg-max hangs on one fp32 rounding
    for z in pre:
        assert z.detach().abs().min().item() > 1e-5, "a pre-activation within 1e-5 of zero: choose another seed"
    jbest = torch.gather(idx.unsqueeze(1).expand(B, 64, n, k), 3, arg.unsqueeze(-1))       # neighbour index of the arg-max
    rival = (idx.unsqueeze(1).expand(B, 64, n, k) != jbest) & ((out.unsqueeze(-1) - h).detach() < 1e-5)
    assert not bool(rival.any()), "a runner-up from another neighbour within 1e-5 of a max: choose another seed"
    (out * case["w"]).sum().backward()
    ref = dict(out=out.detach(), dpq=pq.grad, g1=bn1.weight.grad, b1=bn1.bias.grad, rm1=bn1.running_mean, rv1=bn1.running_var,
               mean1=y1.detach().mean((0, 2, 3)), var1=y1.detach().var((0, 2, 3), unbiased=False))
    if two:
        ref.update(dw2=w2.grad, g2=bn2.weight.grad, b2=bn2.bias.grad, rm2=bn2.running_mean, rv2=bn2.running_var)
    return ref


_REF_CACHE = {}


def _reference_cached(key, two):
    if key not in _REF_CACHE:
        case = _make_case(*key)
        _REF_CACHE[key] = (case, _reference(case, two))
    return _REF_CACHE[key]


def _bn32(cls, gamma, beta, run):
    bn = cls(64, eps=EPS).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(run[0]), bn.running_var.copy_(run[1])
    return bn


def _run_gpu(case, two, idx=None, lo=0, hi=None, bn_cls=torch.nn.BatchNorm2d):
    from geometric_aware_dense_matching_amd import ops
    hi = case["B"] if hi is None else hi
    idx = case["idx"] if idx is None else idx
    pq = case["pq"][lo:hi].cuda().requires_grad_(True)
    bn1 = _bn32(bn_cls, *case["bns"][0], case["run"][0])
    bn2 = _bn32(bn_cls, *case["bns"][1], case["run"][1]) if two else None
    w2 = case["w2"].cuda().view(64, 64, 1, 1).requires_grad_(True) if two else None       # as nn.Conv2d holds it
    out = ops.edge_block_train(pq, idx[lo:hi].cuda(), bn1, w2, bn2, slope=SLOPE)
    (out * case["w"][lo:hi].float().cuda()).sum().backward()
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dpq=pq.grad, g1=bn1.weight.grad, b1=bn1.bias.grad, rm1=bn1.running_mean, rv1=bn1.running_var,
               nbt=[int(bn1.num_batches_tracked)] + ([int(bn2.num_batches_tracked)] if two else []))
    if two:
        got.update(dw2=w2.grad.view(64, 64), g2=bn2.weight.grad, b2=bn2.bias.grad, rm2=bn2.running_mean, rv2=bn2.running_var)
    return got


def _check(got, ref, two, lo=0, hi=None, what=""):
    """The criteria of the stage: output 5e-4 scale, running statistics rtol 1e-5 / atol 1e-6, gradients 1e-4 scale per tensor."""
    scale = lambda t: max(1.0, t.abs().max().item())
    sl = slice(lo, hi)
    worst = {}
    err = (got["out"].cpu().double() - ref["out"][sl]).abs().max().item()
    worst["out"] = err / (5e-4 * scale(ref["out"]))
    dpq = got["dpq"].cpu().double()
    worst["dP"] = (dpq[..., :64] - ref["dpq"][sl][..., :64]).abs().max().item() / (1e-4 * scale(ref["dpq"][..., :64]))
    worst["dQ"] = (dpq[..., 64:] - ref["dpq"][sl][..., 64:]).abs().max().item() / (1e-4 * scale(ref["dpq"][..., 64:]))
    names = ["g1", "b1"] + (["dw2", "g2", "b2"] if two else [])
    for name in names:
        worst[name] = (got[name].cpu().double() - ref[name]).abs().max().item() / (1e-4 * scale(ref[name]))
    print("%s error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in worst.items())))
    for name, v in worst.items():
        assert v < 1.0, (name, v)
    for name in ["rm1", "rv1"] + (["rm2", "rv2"] if two else []):
        assert torch.allclose(got[name].cpu().double(), ref[name], rtol=1e-5, atol=1e-6), name
    return worst


# (B, C, n, k, two convolutions): the first stage (ragged last workgroup, fewer than four points in the last wave pass), k = 20 (80 edges
# per four points = five MFMA tiles, a 60-edge tail), the third stage (batch stride, three workgroups); seeds whose fragile set is empty
STAGE_CASES = ([(1, 9, 70, 16, True, s) for s in (202, 206, 229)] + [(1, 64, 67, 20, True, s) for s in (200, 209, 211)]
               + [(2, 64, 130, 16, False, s) for s in (210, 250)])


@pytest.mark.parametrize("B,C,n,k,two,seed", STAGE_CASES)
def test_edge_block_train_vs_fp64_autograd(B, C, n, k, two, seed):
    case, ref = _reference_cached((B, C, n, k, seed), two)
    got = _run_gpu(case, two)
    _check(got, ref, two, what="(%d,%d,%d,%d,%s) seed %d" % (B, C, n, k, two, seed))
    assert got["nbt"] == [1] * (2 if two else 1)
    # point 11 is nobody's neighbour: its row of the neighbour half receives no atomic at all
    assert bool((got["dpq"][:, 11, :64] == 0).all())
    # an index outside [0, n) is clamped, not followed: output bit for bit, gradients up to the order of the atomics
    bad = case["idx"].clone()
    bad[:, :, 1] = torch.where(torch.arange(n) % 2 == 0, torch.tensor(-5), torch.tensor(n + 7))
    a = _run_gpu(case, two, idx=bad)
    b = _run_gpu(case, two, idx=bad.clamp(0, n - 1))
    assert torch.equal(a["out"], b["out"])
    for name in ["dpq", "g1", "b1"] + (["dw2", "g2", "b2"] if two else []):
        assert (a[name] - b[name]).abs().max().item() <= 1e-6 * max(1.0, b[name].abs().max().item()), name


def test_edge_block_train_batch_statistics_and_forward_kernel():
    """The statistics pass against the fp64 moments, and the forward output bit for bit the inference kernel's (ops.edge_block) on
    the batch statistics folded into scale and shift."""
    from geometric_aware_dense_matching_amd import _lib, ops
    B, C, n, k, two, seed = STAGE_CASES[3]
    case, ref = _reference_cached((B, C, n, k, seed), two)
    got = _run_gpu(case, two)
    pq, idx, w2 = case["pq"].cuda(), case["idx"].int().cuda(), case["w2"].cuda()
    E = float(B * n * k)

    def sums(st1):
        buf = ops._edge_sums_buffer(B, n, k, pq.device)
        ops.check(_lib.lib().gdm_edge_stats_hip(pq.data_ptr(), idx.data_ptr(), st1.data_ptr() if st1 is not None else None,
                                                w2.data_ptr() if st1 is not None else None, SLOPE, B, n, k, buf.data_ptr(), None), "gdm_edge_stats_hip")
        return buf[:-2].view(-1, 128).sum(0).view(64, 2)

    s1 = sums(None)
    assert torch.allclose((s1[:, 0] / E).cpu(), ref["mean1"], rtol=1e-5, atol=1e-6)
    assert torch.allclose((s1[:, 1] / E - (s1[:, 0] / E) ** 2).cpu(), ref["var1"], rtol=1e-5, atol=1e-6)
    (g1, b1), (g2, b2) = case["bns"]
    st1 = ops._edge_bn_fold(s1, E, g1.float().cuda(), b1.float().cuda(), EPS, 0.1, None, None)
    st2 = ops._edge_bn_fold(sums(st1), E, g2.float().cuda(), b2.float().cuda(), EPS, 0.1, None, None)
    out = ops.edge_block(pq, idx, st1[0], st1[1], w2, st2[0], st2[1], SLOPE)
    assert torch.equal(out, got["out"])


def test_edge_block_train_refuses_what_it_cannot_do():
    from geometric_aware_dense_matching_amd import ops
    pq = torch.zeros(1, 8, 128, device="cuda")
    idx = torch.zeros(1, 8, 4, dtype=torch.int32, device="cuda")
    bn = torch.nn.BatchNorm2d(64).cuda()
    with pytest.raises(ValueError, match="training mode"):
        ops.edge_block_train(pq, idx, bn.eval())
    with pytest.raises(ValueError, match="go together"):
        ops.edge_block_train(pq, idx, bn.train(), torch.zeros(64, 64, device="cuda"), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_block_train(pq.cpu(), idx, bn.train())


def test_edge_block_train_allocates_no_edge_tensor():
    """Forward + backward at B = 2, n = 4096, k = 16 with two convolutions: the peak grows by less than ONE [B,64,n,k] fp32 tensor (the
    operands and gradients -- pq's gradient, out, the arg-max map, the dW2 slabs -- come to about 0.6 of it; the module path keeps at
    least six such tensors for this stage)."""
    from geometric_aware_dense_matching_amd import ops
    B, n, k = 2, 4096, 16
    g = torch.Generator().manual_seed(5)
    pq = torch.randn(B, n, 128, generator=g).cuda().requires_grad_(True)
    idx = torch.randint(0, n, (B, n, k), generator=g).int().cuda()
    w2 = (torch.randn(64, 64, generator=g) / 8).cuda().requires_grad_(True)
    w = torch.randn(B, 64, n, generator=g).cuda()
    bn1, bn2 = torch.nn.BatchNorm2d(64).cuda().train(), torch.nn.BatchNorm2d(64).cuda().train()

    def step():
        pq.grad = w2.grad = None
        bn1.zero_grad(set_to_none=True), bn2.zero_grad(set_to_none=True)
        (ops.edge_block_train(pq, idx, bn1, w2, bn2) * w).sum().backward()

    step()                                                      # warm-up: library handles, the allocator's first blocks
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    one = B * 64 * n * k * 4
    print("peak growth %.1f MB = %.2f of one [B,64,n,k] tensor" % (growth / 1e6, growth / one))
    assert growth < one
    assert bool(torch.isfinite(pq.grad).all()) and bool(torch.isfinite(w2.grad).all())


def test_edge_block_train_in_a_captured_graph():
    """No host synchronisation inside the Function: forward + backward are captured and the replay equals the eager step (the
    neighbour half of pq's gradient up to the order of its float atomics)."""
    from geometric_aware_dense_matching_amd import ops
    B, C, n, k, _, seed = STAGE_CASES[0]
    case = _make_case(B, C, n, k, seed)
    pq = case["pq"].cuda().requires_grad_(True)
    idx, w = case["idx"].int().cuda(), case["w"].float().cuda()
    w2 = case["w2"].cuda().requires_grad_(True)
    bn1, bn2 = _bn32(torch.nn.BatchNorm2d, *case["bns"][0], case["run"][0]), _bn32(torch.nn.BatchNorm2d, *case["bns"][1], case["run"][1])
    params = [pq, w2, bn1.weight, bn1.bias, bn2.weight, bn2.bias]

    def step():
        out = ops.edge_block_train(pq, idx, bn1, w2, bn2)
        return out, torch.autograd.grad((out * w).sum(), params)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [eager[0].clone()] + [t.clone() for t in eager[1]]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0])
    for a, b in zip(grads, eager[1:]):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item())
    assert int(bn1.num_batches_tracked) == 2                    # the eager step and the replay (capturing runs nothing)


# the third stage's case, and a two-convolution one of B = 2 so that all four sets of sums (two forward, two backward) go through the
# all-reduce: at the third case's shape two layers hold 5e5 pre-activations and about four of them lie within 1e-5 of zero for every
# seed, so the second case is smaller (n = 40); its seed was searched on the CPU with the same precondition (307, 312, 344 pass)
SYNC_CASES = [STAGE_CASES[7], (2, 64, 40, 16, True, 307)]


def _sync_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from geometric_aware_dense_matching_amd import ops
        torch.cuda.set_device(0)
        for B, C, n, k, two, seed in SYNC_CASES:
            case = _make_case(B, C, n, k, seed)
            ref = _reference(case, two)                         # fp64 over the WHOLE batch
            lo, hi = rank * B // world, (rank + 1) * B // world
            got = _run_gpu(case, two, lo=lo, hi=hi, bn_cls=torch.nn.SyncBatchNorm)
            assert ops._sync_group(torch.nn.SyncBatchNorm(64).cuda()) is not None
            # local parameter-gradient sums -> whole batch (DDP would average them)
            for name in ["g1", "b1"] + (["dw2", "g2", "b2"] if two else []):
                t = got[name].double().cpu()
                dist.all_reduce(t)
                got[name] = t
            _check(got, ref, two, lo=lo, hi=hi, what="rank %d two=%s" % (rank, two))
            assert got["nbt"] == [1] * (2 if two else 1)
        if rank == 0:
            out.put("ok")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_edge_block_train_syncbatchnorm_two_ranks_equals_whole_batch():
    """SyncBatchNorm: two ranks (gloo, both on this GPU) with half of a B = 2 batch each == the fp64 restatement over the whole batch --
    outputs, pq's gradient, summed parameter gradients and running statistics at the single-process bounds (SYNC_CASES)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    out = ctx.SimpleQueue()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    assert out.get() == "ok"


def _dgcnn_model(M):
    from geometric_aware_dense_matching_amd.config import make_dgcnn_cfg
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    torch.manual_seed(0)
    model = GeoMatchDGCNN(make_dgcnn_cfg(n_mesh_node=M, dataset="ycbv"), 2, model_points=synthetic.make_model_points(2, M, 269.573))
    model.model_emb.k = 20
    return model.cuda().train()


def test_training_step_fused_path_equals_module_path(monkeypatch):
    """One whole training step of the variant (N = 512, M = 384, k = 16 / 20, B = 2): `train_path = "fused"` against the module path
    with the fused path's six graphs injected (feature-space graphs differ at fp32 near-ties otherwise: a property of the kNN) --
    loss, running variances, relative L2 distance d over all parameter gradients, against the distance `noise` of the module path
    from itself on an input moved by one fp32 rounding.  The tight check is
    tests/test_gpu_step_compare.py::test_dgcnn_step_on_the_fused_path_equals_the_module_path_per_parameter: the same A/B per parameter."""
    from geometric_aware_dense_matching_amd import dgcnn, train_lm
    M, N, B = 384, 512, 2
    dev = torch.device("cuda", 0)
    model = _dgcnn_model(M)
    assert model.train_path == "modules"
    state = {k: v.clone() for k, v in model.state_dict().items()}
    ds = train_lm.SyntheticCrops(B, N, M, seed=5)
    batch = torch.utils.data.default_collate([ds[i] for i in range(B)])

    def run(path):
        model.train_path = path
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)                                   # same dropout masks
        out, _ = train_lm.model_fn_dec(model, batch, dev)
        out["loss"].backward()
        return (float(out["loss"].detach()),
                {k: p.grad.detach().double().clone() for k, p in model.named_parameters() if p.grad is not None},
                {k: v.double().clone() for k, v in model.state_dict().items() if k.endswith("running_var")})

    graphs = []
    real_knn_fused = dgcnn.knn_fused

    def recording(feat, k):
        graphs.append(real_knn_fused(feat, k))
        return graphs[-1]

    monkeypatch.setattr(dgcnn, "knn_fused", recording)
    l1, g1, s1 = run("fused")
    assert len(graphs) == 6 and [g.shape[2] for g in graphs] == [16] * 3 + [20] * 3
    monkeypatch.setattr(dgcnn, "knn_fused", real_knn_fused)
    replay = []
    monkeypatch.setattr(dgcnn, "knn", lambda x, k: replay.pop(0))
    replay[:] = list(graphs)
    l0, g0, s0 = run("modules")
    assert not replay
    cld0 = batch["cld_rgb_nrm"].clone()
    sign = torch.from_numpy(np.where(np.random.RandomState(3).rand(*cld0.shape) < 0.5, -1.0, 1.0).astype(np.float32))
    batch["cld_rgb_nrm"] = cld0 * (1.0 + sign * 2.0 ** -23)
    replay[:] = list(graphs)
    ln, gn, _ = run("modules")
    batch["cld_rgb_nrm"] = cld0
    den = sum((v ** 2).sum().item() for v in g0.values()) ** 0.5
    dist = lambda g: sum(((g[k] - g0[k]) ** 2).sum().item() for k in g0) ** 0.5 / den
    d, noise = dist(g1), dist(gn)
    print("DGCNN training A/B: loss modules %.6f fused %.6f, gradient distance d %.3e, one-rounding input noise %.3e, %d gradients"
          % (l0, l1, d, noise, len(g0)))
    assert np.isfinite(l0) and set(g0) == set(g1) and len(g0) > 60
    assert abs(l1 - l0) < 1e-4 * abs(l0), (l0, l1)
    for k in s0:
        assert torch.allclose(s0[k], s1[k], rtol=5e-2, atol=1e-3), k
    assert d < max(3e-2, 10.0 * noise), (d, noise)


def test_train_path_selection_and_state_dict_names():
    from geometric_aware_dense_matching_amd import train_lm, train_ycb
    a = train_ycb.build_parser().parse_args("-state=train -cls_id=16 --model-variant dgcnn --dgcnn-train-path fused --n-mesh 256".split())
    assert a.dgcnn_train_path == "fused"
    fused = train_lm.build_model(a, 16)
    a.dgcnn_train_path = "modules"
    modules = train_lm.build_model(a, 16)
    assert fused.train_path == "fused" and modules.train_path == "modules"
    assert list(fused.state_dict()) == list(modules.state_dict())
    with pytest.raises(SystemExit):
        train_ycb.build_parser().parse_args("--dgcnn-train-path eager".split())
    fused.train_path = "eager"
    x = torch.from_numpy(synthetic.make_batch(seed=8, batch=2, n_points=256)["cld_rgb_nrm"]).cuda()
    with pytest.raises(ValueError, match="train_path"):
        fused.cuda().train()(dict(cld_rgb_nrm=x))


def test_entry_points_train_on_the_fused_path_then_test(tmp_path):
    """`train_ycb -state=train --model-variant dgcnn --dgcnn-train-path fused --max-iters 3` writes a checkpoint that loads into a model
    on the module path, `-state=test` runs on it, and the same three iterations run with --graph-train."""
    from geometric_aware_dense_matching_amd import config, train_lm, train_ycb
    from geometric_aware_dense_matching_amd.checkpoint import load_checkpoint
    cls_id = 16
    common = "--n-points 1024 --n-mesh 256 --synthetic-items 4 --model-variant dgcnn"
    train_args = ("-state=train -cls_id=%d --deterministic --batch-size 2 --epochs 2 --save-every 1 --log-every 1 --max-iters 3 "
                  "--dgcnn-train-path fused %s" % (cls_id, common))
    a = train_ycb.build_parser().parse_args((train_args + " --log-dir %s" % tmp_path).split())
    ds = config.dataset_config(a.dataset_name)
    trainer = train_lm.train(a)
    assert trainer.model.train_path == "fused"
    assert len(trainer.history) == 3 and all(np.isfinite(h).all() for h in trainer.history)
    name = ds["objs"][cls_id]
    assert os.path.exists(os.path.join(str(tmp_path), name, "geomatch.pth.tar"))           # written after the first epoch (two iterations)
    t = train_ycb.build_parser().parse_args(("-state=test -cls_id=%d -checkpoint %s --batch-size 4 %s" % (cls_id, tmp_path, common)).split())
    model = train_lm.build_model(t, cls_id, cache_mesh_in_eval=True).cuda()
    assert model.train_path == "modules"
    assert load_checkpoint(model, None, os.path.join(str(tmp_path), name, "geomatch"), device="cuda", strict=ds["load_strict"]) == 0
    res = train_lm.test(t)
    assert len(res) == 1 and res[0]["best_idx"].shape == (4, 1024) and int(res[0]["best_idx"].max()) < 256
    graph_dir = os.path.join(str(tmp_path), "graphed")
    b = train_ycb.build_parser().parse_args((train_args + " --graph-train --log-dir %s" % graph_dir).split())
    graphed = train_lm.train(b)
    assert len(graphed.history) == 3 and all(np.isfinite(h).all() for h in graphed.history)
