"""The first mesh layer with its weight slice in LDS (spline_direct_lds_kernel) against the kernel it replaces
(spline_direct_vec_kernel, weight rows from global memory), through the C entry gdm_spline_direct3_hip and its weights_in_lds
argument.  The two kernels instantiate one body (csrc/gdm_spline.hip spline_direct_vertex4) and differ only in where a weight row
comes from, so all three outputs -- out f32[M,C], out_t f32[C,M] and the packed split-bf16 operand of the next layer -- are held to
torch.equal, not to a tolerance.

Shapes: the vertex run of a workgroup is 128 and a pass walks 64 vertices, so M = 1 (one thread quad), M = 200 (a partial second run,
a partial pass) and M = 1000 (eight runs) cover the run arithmetic; Cin = 3, 9, 16 the guarded tail of the q loop and the largest
LDS slice (128,000 B); in-degrees 0 .. 9 the edge loop, a vertex without edges included; attr = 0.0 and 1.0 the wrap of
(floor + 1) % 5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = 5


def _case(M, Cin, C, degs, seed, edge_attr=None):
    """A hand-made CSR graph (degs[i] in-edges of vertex i, sources drawn anywhere) with random inputs, weights, root and bias."""
    rs = np.random.RandomState(seed)
    degs = np.asarray(degs, dtype=np.int64)
    assert degs.shape == (M,)
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    E = int(rowptr[-1])
    src = rs.randint(0, M, size=max(E, 1)).astype(np.int32)
    attr = rs.rand(max(E, 1), 3).astype(np.float32)
    if edge_attr is not None:
        attr[:len(edge_attr)] = edge_attr
    d = "cuda"
    return dict(M=M, Cin=Cin, C=C, x=torch.from_numpy(rs.randn(M, Cin).astype(np.float32)).to(d),
                weight=torch.from_numpy((rs.randn(KS ** 3, Cin, C) / 3).astype(np.float32)).to(d),
                rowptr=torch.from_numpy(rowptr).to(d), src=torch.from_numpy(src).to(d), attr=torch.from_numpy(attr).to(d),
                root_t=torch.from_numpy((rs.randn(Cin, C) / 3).astype(np.float32)).to(d),
                bias=torch.from_numpy(rs.randn(C).astype(np.float32)).to(d))


def _run(c, relu, lds, packed=True, root=True, bias=True):
    """(out, out_t, packed) of one launch; every buffer starts as NaN / 0xFF-free zeros so that an unwritten element shows."""
    from geometric_aware_dense_matching_amd import _lib
    M, C = c["M"], c["C"]
    out = torch.full((M, C), float("nan"), device="cuda")
    out_t = torch.full((C, M), float("nan"), device="cuda")
    pk = torch.zeros(_lib.lib().gdm_conv3x3_act_bytes(1, C, 1, M), dtype=torch.uint8, device="cuda") if packed else None
    _lib.call("gdm_spline_direct3_hip", c["x"], c["weight"], c["rowptr"], c["src"], c["attr"], c["root_t"] if root else None,
              c["bias"] if bias else None, M, c["Cin"], C, KS, int(relu), out, out_t, pk, int(lds))
    torch.cuda.synchronize()
    return out, out_t, pk


def _same(c, relu, **kw):
    new, old = _run(c, relu, True, **kw), _run(c, relu, False, **kw)
    for name, a, b in zip(("out", "out_t", "packed"), new, old):
        if a is None:
            continue
        assert not torch.isnan(a).any() if a.dtype.is_floating_point else True, name
        assert torch.equal(a, b), "%s differs between the LDS and the global-memory kernel" % name
    assert torch.equal(new[0], new[1].t()), "out_t is not the transpose of out"
    return new


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("Cin", [3, 9, 16])
@pytest.mark.parametrize("M", [1, 200])
def test_lds_kernel_equals_the_global_memory_kernel(M, Cin, relu):
    degs = np.full(M, 4) if M > 1 else np.array([3])
    _same(_case(M, Cin, 128, degs, 100 * M + Cin), relu)


@pytest.mark.parametrize("relu", [True, False])
def test_in_degrees_0_to_9_and_attr_on_the_wrap(relu):
    """M = 1000 with in-degrees 0 .. 9 (vertex 0 and every tenth one have no edge: their message is 0, the result root + bias), and
    edge attributes exactly 0.0 and 1.0 in every axis combination: floor = 4 at 1.0, so the upper corner wraps to index 0 with
    weight 0."""
    M = 1000
    degs = np.arange(M) % 10
    wrap = np.array([[a, b, c] for a in (0.0, 1.0) for b in (0.0, 1.0) for c in (0.0, 1.0)] + [[1.0, 0.5, 0.25], [0.25, 1.0, 0.0]],
                    dtype=np.float32)
    c = _case(M, 9, 128, degs, 7, edge_attr=wrap)
    out, _, _ = _same(c, relu)
    no_edge = torch.from_numpy(np.nonzero(degs == 0)[0]).cuda()
    want = c["x"][no_edge].double() @ c["root_t"].double() + c["bias"].double()
    want = want.clamp(min=0) if relu else want
    assert (out[no_edge].double() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())


def test_without_root_bias_and_packed_output():
    _same(_case(200, 9, 128, np.full(200, 4), 11), True, packed=False, root=False, bias=False)


def test_lds_kernel_against_fp64():
    """The shared body itself against the layer's definition in fp64 (1e-5 * max |want|, the bound of the existing direct-layer
    tests): mean over the in-edges of sum_s b_s (x_j . W[wi_s]), + x_i . W_root + bias, ReLU."""
    M, Cin, C = 200, 9, 128
    c = _case(M, Cin, C, np.arange(M) % 6, 5)
    out, _, _ = _run(c, True, True)
    rowptr, src, attr = c["rowptr"].cpu().numpy(), c["src"].cpu().numpy(), c["attr"].cpu().numpy().astype(np.float64)
    x, w = c["x"].cpu().double().numpy(), c["weight"].cpu().double().numpy()
    want = np.zeros((M, C))
    for i in range(M):
        for e in range(rowptr[i], rowptr[i + 1]):
            v = np.float32(attr[e]).astype(np.float32) * np.float32(KS - 1)
            fl = np.floor(v).astype(np.int64)
            fr = (v - np.floor(v)).astype(np.float64)
            for s in range(8):
                kd = [(s >> d) & 1 for d in range(3)]
                wi = sum(((fl[d] + kd[d]) % KS) * KS ** d for d in range(3))
                b = np.prod([fr[d] if kd[d] else 1.0 - fr[d] for d in range(3)])
                want[i] += b * (x[src[e]] @ w[wi])
        if rowptr[i + 1] > rowptr[i]:
            want[i] /= rowptr[i + 1] - rowptr[i]
    want = np.maximum(want + x @ c["root_t"].cpu().double().numpy() + c["bias"].cpu().double().numpy(), 0.0)
    err = np.abs(out.cpu().double().numpy() - want).max()
    assert err < 1e-5 * max(1.0, np.abs(want).max()), err


def test_a_shape_the_lds_kernel_refuses_runs_on_the_old_one():
    """C = 64 is outside the LDS kernel (it is built for the 128-channel layer): weights_in_lds = 1 still gives the global-memory
    kernel's result, for out and out_t (C = 64 has no packed form)."""
    _same(_case(133, 9, 64, np.full(133, 4), 3), True, packed=False)
