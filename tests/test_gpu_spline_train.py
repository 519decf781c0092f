"""GPU: training the mesh branch on the edge-grouped SplineConv (`SplineCNN_Mesh.train_path = "grouped"`): the pair-gradient gather,
the segment sum of the input gradient and the grouped weight gradient (csrc/gdm_spline.hip) against an fp64 restatement of the operator
under autograd, and the path against the dense one inside the branch, under graph capture and in a model step.

Shapes (the smallest that show each hazard): M = 12 (most of the 125 kernel indices empty: an unwritten dW[k] shows in poison-filled
outputs), M = 700 (kernel indices spanning more than one 256-row tile), M = 2048 (the grouped inference test's shape), and the
hand-made CSR of test_spline_pairs_cpu (a degree-0 vertex, a degree-7 vertex, a pair shared by identical edges).  build_mesh_graph
normalises by the largest offset, so every kNN graph has a pseudo-coordinate of exactly 0.0 or 1.0: a zero-basis wrapped corner.

Bounds are the project's standing ones for this operand class: outputs 1e-5 * max(1, |ref|max) (test_spline_grouped_form_equals_dense_form),
gradients 1e-4 * max(1, |ref|max) per tensor (_check of test_gpu_dgcnn_train)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from geometric_aware_dense_matching_amd import _lib, ops, splinecnn, synthetic  # noqa: E402
from test_spline_pairs_cpu import check_inverse_maps, hand_made_csr  # noqa: E402

OUT_BOUND, GRAD_BOUND = 1e-5, 1e-4
_graphs = {}


def _graph(case):
    """(rowptr, src, attr, M, pairs) on the GPU, built once per case and left unchanged."""
    if case not in _graphs:
        if case == "hand":
            rowptr, src, attr, M = hand_made_csr()
            rowptr, src, attr = rowptr.cuda(), src.cuda(), attr.cuda()
        else:
            M = int(case[1:])
            torch.manual_seed(M)
            pos = torch.rand(M, 3, device="cuda")
            ei, ea = splinecnn.build_mesh_graph(pos, k=4)
            order = torch.argsort(ei[1], stable=True)
            rowptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
            rowptr[1:] = torch.cumsum(torch.bincount(ei[1][order], minlength=M), 0).to(torch.int32)
            src, attr = ei[0][order].to(torch.int32).contiguous(), ea[order].contiguous()
            assert bool(((attr == 0.0) | (attr == 1.0)).any())
        pairs = splinecnn.build_spline_pairs(src, attr, M, rowptr=rowptr)
        _graphs[case] = (rowptr, src, attr, M, pairs)
    return _graphs[case]


def _pre64(x, W, Wr, b, rowptr, src, attr):
    """The operator of the header of gdm_spline.hip in fp64 torch, before the ReLU: out_i = mean_{e -> i} sum_s b_s x_j W[wi_s] + x_i
    W_root + bias.  Returns (pre f64[M,C], xw f64[M,125,C] -- the table whose gradient holds gY at the (source, kernel index) pairs)."""
    M, C = x.shape[0], W.shape[2]
    deg = (rowptr[1:] - rowptr[:-1]).long()
    tgt = torch.repeat_interleave(torch.arange(M, device=x.device), deg)
    v = attr.double() * 4.0
    fl = torch.floor(v)
    fr = v - fl
    xw = (x @ W.permute(1, 0, 2).reshape(x.shape[1], -1)).view(M, 125, C)
    xw.retain_grad()
    msg = 0
    for s in range(8):
        wi = sum(((fl[:, d].long() + ((s >> d) & 1)) % 5) * 5 ** d for d in range(3))
        bs = torch.stack([fr[:, d] if (s >> d) & 1 else 1.0 - fr[:, d] for d in range(3)]).prod(0)
        msg = msg + bs[:, None] * xw[src.long(), wi]
    agg = torch.zeros(M, C, dtype=torch.float64, device=x.device).index_add(0, tgt, msg) / deg.clamp(min=1)[:, None]
    return agg + x @ Wr.t() + b, xw


def _report(what, errs):
    print("%s error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in errs.items())))
    for name, v in errs.items():
        assert v < 1.0, (what, name, v)


def _ratio(got, ref, bound):
    return (got.double() - ref).abs().max().item() / (bound * max(1.0, ref.abs().max().item()))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("cin", [128, 9])
@pytest.mark.parametrize("case", ["m12", "m700", "m2048", "hand"])
def test_kernels_against_fp64(case, cin, relu):
    """gY, dX, dW, root and bias gradients of one SplineConv layer on the grouped training path against fp64 autograd; the forward is the
    eval forward bit for bit; a second backward gives the same bits; outputs written into poison-filled buffers are fully written.

    The ReLU mask of the reference is taken from the layer's own fp32 output, as the backward under test takes it (g = go * (out > 0)):
    where the fp64 pre-activation lies within the forward tolerance of zero the two signs may differ, which is a property of comparing
    a ReLU across precisions and not of these kernels; the forward check holds the output itself to the fp64 ReLU."""
    rowptr, src, attr, M, pairs = _graph(case)
    check_inverse_maps(pairs, rowptr, src, M)
    torch.manual_seed(7 * M + cin + int(relu))
    conv = splinecnn.SplineConv(cin, 128).cuda()
    conv.bias.data.normal_(0, 0.1)
    x = torch.randn(M, cin, device="cuda", requires_grad=cin == 128)
    go = torch.randn(M, 128, device="cuda")
    assert conv.train_grouped_ok(x, pairs)

    def run():
        for t in (x, conv.weight, conv.lin.weight, conv.bias):
            t.grad = None
        out = conv.forward_train_grouped(x, rowptr, src, attr, relu, pairs)
        out.backward(go)
        grads = dict(dW=conv.weight.grad.clone(), root=conv.lin.weight.grad.clone(), bias=conv.bias.grad.clone())
        if cin == 128:
            grads["dX"] = x.grad.clone()
        return out.detach(), grads

    out, grads = run()
    out2, grads2 = run()
    assert torch.equal(out, out2)
    for k in grads:                                           # no atomics, fixed summation order
        assert torch.equal(grads[k], grads2[k]), k
    with torch.no_grad():
        assert torch.equal(out, conv(x, rowptr, src, attr, relu=relu, pairs=pairs))           # the launches of inference

    # the three kernels through the C ABI into poison-filled outputs: every element is written
    L = _lib.lib()
    R = pairs["rowidx"].shape[0]
    nan = float("nan")
    gy = torch.full((R, 128), nan, device="cuda")
    _lib.check(L.gdm_spline_pairs_grad_hip(go.data_ptr(), out.data_ptr() if relu else None, pairs["pair_ptr"].data_ptr(), pairs["pair_ec"].data_ptr(),
                                           pairs["basis"].data_ptr(), pairs["tgt"].data_ptr(), pairs["inv_deg"].data_ptr(), R, 128, gy.data_ptr(),
                                           None, ops._stream()), "gdm_spline_pairs_grad_hip")
    dw = torch.full((125, cin, 128), nan, device="cuda")
    xd = x.detach()
    part = torch.full((R // 256, cin, 128), nan, device="cuda")
    _lib.check(L.gdm_spline_wgrad_hip(xd.data_ptr(), pairs["rowidx"].data_ptr(), gy.data_ptr(), pairs["tile_co0"].data_ptr(),
                                      pairs["blk_start"].data_ptr(), pairs["blk_rows"].data_ptr(), 125, R, cin, 128, part.data_ptr(),
                                      dw.data_ptr(), ops._stream()), "gdm_spline_wgrad_hip")
    assert bool(torch.isfinite(gy).all()) and torch.equal(dw, grads["dW"])
    real = torch.zeros(R, dtype=torch.bool)
    for s0, n in zip(pairs["blk_start"].tolist(), pairs["blk_rows"].tolist()):
        real[s0: s0 + n] = True
    real = real.cuda()
    assert not bool(dw[pairs["blk_rows"] == 0].any())         # an empty kernel index is written as zeros
    assert not bool(gy[~real].any())                          # and so are the padding rows of gY
    if case == "m12":
        assert int((pairs["blk_rows"] == 0).sum()) > 0
    if case == "m700":
        assert int(pairs["blk_rows"].max()) > 256
    if cin == 128:
        seg = torch.full((M, 128), nan, device="cuda")
        z = torch.randn(R, 128, device="cuda")
        _lib.check(L.gdm_spline_segment_sum_hip(z.data_ptr(), pairs["src_ptr"].data_ptr(), pairs["src_rows"].data_ptr(), None, M, 128,
                                                seg.data_ptr(), ops._stream()), "gdm_spline_segment_sum_hip")
        want = torch.zeros(M, 128, dtype=torch.float64, device="cuda").index_add(0, pairs["rowidx"].long()[real], z.double()[real])
        _report("%s segment sum" % case, {"sum": _ratio(seg, want, GRAD_BOUND)})

    # fp64 restatement under autograd
    x64 = x.detach().double().requires_grad_(True)
    W64, Wr64, b64 = (t.detach().double().requires_grad_(True) for t in (conv.weight, conv.lin.weight, conv.bias))
    pre, xw = _pre64(x64, W64, Wr64, b64, rowptr, src, attr)
    ref_out = torch.relu(pre) if relu else pre
    mask = (out > 0).double() if relu else torch.ones_like(pre)
    (pre * mask * go.double()).sum().backward()
    kidx = pairs["tile_co0"].long().repeat_interleave(256) // 128
    gy_ref = xw.grad[pairs["rowidx"].long(), kidx] * real[:, None]
    errs = {"out": _ratio(out, ref_out.detach(), OUT_BOUND), "gY": _ratio(gy, gy_ref, GRAD_BOUND), "dW": _ratio(grads["dW"], W64.grad, GRAD_BOUND),
            "root": _ratio(grads["root"], Wr64.grad, GRAD_BOUND), "bias": _ratio(grads["bias"], b64.grad, GRAD_BOUND)}
    if cin == 128:
        errs["dX"] = _ratio(grads["dX"], x64.grad, GRAD_BOUND)
    _report("%s SplineConv(%d,128) relu=%d" % (case, cin, relu), errs)


def _mesh(M, dropout=0.1, layers=3, seed=0):
    torch.manual_seed(seed)
    m = splinecnn.SplineCNN_Mesh({"n_mesh_node": M}, 1, num_mesh_layers=layers, dropout=dropout, model_points=synthetic.make_model_points(1, M))
    for c in m.mesh_convs:
        c.bias.data.normal_(0, 0.1)
    return m.cuda().train()


def _branch_step(mesh, w, seed=3):
    mesh.zero_grad(set_to_none=True)
    torch.manual_seed(seed)                                   # the same dropout mask on every path
    out = mesh()
    (out * w).sum().backward()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in mesh.named_parameters()}


def test_whole_branch_grouped_equals_dense():
    """SplineCNN_Mesh, three layers, 700 vertices, train mode, fixed seed: output and every parameter gradient of "grouped" against
    "dense" within the two bounds."""
    M = 700
    mesh = _mesh(M)
    w = torch.randn(128, M, device="cuda")
    assert mesh.train_path == "dense"
    out0, g0 = _branch_step(mesh, w)
    mesh.train_path = "grouped"
    assert mesh._train_grouped_ok()
    out1, g1 = _branch_step(mesh, w)
    assert set(g0) == set(g1) and len(g0) == 11
    errs = {"out": _ratio(out1, out0.double(), OUT_BOUND)}
    for k in g0:
        errs[k.replace("mesh_convs.", "c")] = _ratio(g1[k], g0[k].double(), GRAD_BOUND)
    _report("mesh branch grouped vs dense", errs)


def _autograd_nodes(t):
    """Names of the autograd nodes behind t, counted."""
    from collections import Counter
    seen, stack, names = set(), [t.grad_fn], Counter()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names[type(fn).__name__] += 1
        stack.extend(f for f, _ in fn.next_functions)
    return names


def test_default_path_is_the_old_branch():
    """train_path untouched, nothing patched: the module's step against the dense branch called directly (SplineConv.forward under
    autograd, torch.cat, dropout, mesh_final).  The output is torch.equal and the recorded autograd graphs are the same nodes, three
    _SplineAggregate backwards and no Function of the grouped path.  The gradients that do not pass through the dense backward's atomicAdd
    (mesh_final, the last layer's root weight and bias) are torch.equal.

    The other seven cannot be held to torch.equal: spline_aggregate_bwd_kernel adds up to nine terms per table entry in whatever order
    the atomics land (at M = 128: 301 (source, kernel index) pairs with three or more nonzero uses), so the old branch differs from
    ITSELF from run to run in exactly these seven tensors -- measured on an MI355X at M = 32 .. 700, four runs each, outputs equal
    every time.  They are held to the reordering of an fp32 sum, i.e. the standing gradient bound of this file."""
    import torch.nn.functional as F
    M = 128
    mesh = _mesh(M, seed=1)
    assert "train_path" not in mesh.__dict__ and type(mesh).train_path == "dense"
    w = torch.randn(128, M, device="cuda")
    mesh.zero_grad(set_to_none=True)
    torch.manual_seed(3)
    out = mesh()
    nodes = _autograd_nodes(out)
    (out * w).sum().backward()
    g = {k: p.grad.detach().clone() for k, p in mesh.named_parameters()}
    mesh.zero_grad(set_to_none=True)
    rowptr, src, attr = mesh._ensure_graph()
    torch.manual_seed(3)
    feats = [mesh.mesh_graph_x]
    for conv in mesh.mesh_convs:
        feats.append(conv(feats[-1], rowptr, src, attr, relu=True, pairs=mesh._pairs))
    old = mesh.mesh_final(F.dropout(torch.cat(feats, dim=-1), p=mesh.dropout, training=True)).transpose(0, 1)
    assert _autograd_nodes(old) == nodes and nodes["_SplineAggregateBackward"] == 3
    assert not any("Grouped" in n or "Direct" in n for n in nodes)
    (old * w).sum().backward()
    assert torch.equal(out.detach(), old.detach())
    exact = ("mesh_final.weight", "mesh_final.bias", "mesh_convs.2.lin.weight", "mesh_convs.2.bias")
    errs = {}
    for k, p in mesh.named_parameters():
        if k in exact:
            assert torch.equal(g[k], p.grad), k
        else:
            errs[k.replace("mesh_convs.", "c")] = _ratio(g[k], p.grad.double(), GRAD_BOUND)
    assert len(errs) == 7
    _report("default path vs the old branch (atomic order only)", errs)


def test_silent_dense_path_where_grouped_is_not_built():
    """eval mode / no_grad keep their inference paths, an unknown value raises, and a module whose layers the path does not serve takes
    the dense branch."""
    mesh = _mesh(128, seed=2)
    mesh.train_path = "grouped"
    assert mesh._ensure_graph() is not None and "pair_ptr" not in mesh._pairs        # the inverse maps are not built for other users ...
    mesh.eval()
    with torch.no_grad():
        mesh()
    assert "pair_ptr" not in mesh._pairs and not mesh._train_grouped_ok() and "pair_ptr" not in mesh._pairs
    mesh.train()
    assert mesh._train_grouped_ok() and "pair_ptr" in mesh._pairs                    # ... but the first time the path is taken
    with torch.no_grad():
        assert not mesh._train_grouped_ok()
    mesh.eval()
    assert not mesh._train_grouped_ok()
    mesh.train()
    mesh.train_path = "table"
    with pytest.raises(ValueError, match="train_path"):
        mesh()
    torch.manual_seed(2)
    wide = splinecnn.SplineCNN_Mesh({"n_mesh_node": 128}, 1, out_channels=64, model_points=synthetic.make_model_points(1, 128)).cuda().train()
    wide.train_path = "grouped"
    out = wide()
    assert not wide._train_grouped_ok() and out.shape == (64, 128) and out.requires_grad


def test_backward_reads_the_weights_of_its_forward():
    """The input gradient multiplies by the weights the forward saw: an in-place update between forward and backward (a second forward,
    optimizer.step(), then this backward) is refused by autograd's version check instead of giving a dX of the new weights."""
    rowptr, src, attr, M, pairs = _graph("m700")
    torch.manual_seed(11)
    conv = splinecnn.SplineConv(128, 128).cuda()
    x = torch.randn(M, 128, device="cuda", requires_grad=True)
    go = torch.randn(M, 128, device="cuda")
    out = conv.forward_train_grouped(x, rowptr, src, attr, True, pairs)
    out.backward(go, retain_graph=True)
    dx = x.grad.clone()
    x.grad = None
    out.backward(go, retain_graph=True)                       # the cached pack serves the same weights again
    assert torch.equal(x.grad, dx)
    with torch.no_grad():
        conv.weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward(go)


def test_graph_capture_replays_the_eager_gradients():
    """Forward + backward of the branch on "grouped" captured once (single stream): the replayed gradients are the eager ones."""
    M = 700
    mesh = _mesh(M, dropout=0.0, seed=4)                     # a captured dropout advances its own generator offset: not what is compared
    mesh.train_path = "grouped"
    w = torch.randn(128, M, device="cuda")
    with ops.buffer_pool(ops.BufferPool()):
        out_e, g_e = _branch_step(mesh, w)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _branch_step(mesh, w)
        torch.cuda.current_stream().wait_stream(side)
        mesh.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_g = mesh()
            (out_g * w).sum().backward()
        for p in mesh.parameters():
            p.grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out_g.detach(), out_e)
    for k, p in mesh.named_parameters():
        assert torch.equal(p.grad, g_e[k]), k


def test_model_step_grouped_loss_equals_dense():
    """One GeoMatch training step at the smallest shape of test_gpu_train (M = 512, N = 1024, B = 2): --mesh-train-path grouped against
    dense, loss within 1e-4 relative."""
    from geometric_aware_dense_matching_amd import train_lm
    M, N, B = 512, 1024, 2
    dev = torch.device("cuda", 0)
    args = train_lm.build_parser().parse_args(("-cls_id=1 --n-points %d --n-mesh %d --mesh-train-path grouped" % (N, M)).split())
    torch.manual_seed(0)
    model = train_lm.build_model(args, 1).to(dev).train()
    assert model.model_emb.train_path == "grouped"
    state = {k: v.clone() for k, v in model.state_dict().items()}
    ds = train_lm.SyntheticCrops(B, N, M, seed=5)
    batch = torch.utils.data.default_collate([ds[i] for i in range(B)])
    taken = []
    real_ok = splinecnn.SplineCNN_Mesh._train_grouped_ok

    def run(path):
        model.model_emb.train_path = path
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        out, _ = train_lm.model_fn_dec(model, batch, dev)
        taken.append(real_ok(model.model_emb))
        out["loss"].backward()
        grads = {k: p.grad.detach().double().clone() for k, p in model.named_parameters() if p.grad is not None}
        return float(out["loss"].detach()), grads

    l1, g1 = run("grouped")
    l0, g0 = run("dense")
    assert taken == [True, False]
    print("GeoMatch step: loss dense %.6f grouped %.6f (relative difference %.2e)" % (l0, l1, abs(l1 - l0) / abs(l0)))
    assert np.isfinite(l0) and set(g0) == set(g1)
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    assert abs(l1 - l0) < 1e-4 * abs(l0), (l0, l1)
