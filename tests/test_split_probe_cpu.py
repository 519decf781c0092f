"""CPU: the one-product probes of tests/split_probe.py before any kernel sees them -- the builders' coverage claims at the shapes of
tests/test_gpu_split_probe.py, the derived tolerance against an fp32 emulation of the three additions in every order, the mutants
the tolerance must reject, and the split model's own distance from the exact product (3 * 2^-16, not the 3 * 2^-18 once documented)."""
import numpy as np
import pytest

import split_probe as S


@pytest.fixture(scope="module")
def sample():
    """200 000 randn operand pairs and their parts."""
    rs = np.random.RandomState(11)
    w, x = rs.randn(200000).astype(np.float32), rs.randn(200000).astype(np.float32)
    return w, x, S.parts(w), S.parts(x)


def test_tolerance_holds_every_order_of_the_three_fp32_additions(sample):
    """hh, hl, lh added into an fp32 zero in all six orders (round to nearest): the worst case is inside 2 * 2^-23 * (|hh| + |hl| + |lh|),
    at about half of it -- the other half is the allowance for a truncating adder."""
    w, x = sample[:2]
    exp, tol = S.one_product(w, x)
    ratio = (np.abs(S.emulate_fp32_orders(w, x) - exp) / tol).max()
    print("fp32 emulation, six orders: largest error / tolerance %.3f" % ratio)
    assert ratio <= 1.0
    assert ratio <= 0.75                                   # round to nearest uses half: a tolerance twice as wide would hide the next test's mutants


def test_the_tolerance_rejects_a_dropped_term(sample):
    """The probe must be able to fail: a kernel that drops lo_w * hi_x, or hi_w * lo_x, or keeps hi * hi alone, is outside the tolerance
    at no less than 99 % of randn outputs.  Recorded, not required: an added lo * lo term and the exact fp32 product."""
    w, x, (hw, lw), (hx, lx) = sample
    exp, tol = S.one_product(w, x)
    mutants = {"lo_w*hi_x dropped": hw * hx + hw * lx, "hi_w*lo_x dropped": hw * hx + lw * hx, "hi only": hw * hx,
               "lo*lo added": exp + lw * lx, "exact fp32 product": (w * x).astype(np.float64)}
    share = {k: float((np.abs(v - exp) > tol).mean()) for k, v in mutants.items()}
    print("share of outputs outside the tolerance: " + ", ".join("%s %.4f" % kv for kv in share.items()))
    for k in ("lo_w*hi_x dropped", "hi_w*lo_x dropped", "hi only"):
        assert share[k] >= 0.99, (k, share[k])


def test_split_model_is_within_three_2_pow_minus_16_of_the_exact_product(sample):
    """|hh + hl + lh - w x| <= 3 * 2^-16 |w x|: a bf16 half-ulp is 2^-8 relative, so |lo| <= 2^-8 |v|, |v - hi - lo| <= 2^-16 |v|, and the
    dropped lo * lo and the two residual terms are 2^-16 |w x| each.  The figure 3 * 2^-18 does NOT hold (asserted too)."""
    w, x, (hw, lw), (hx, lx) = sample
    exact = w.astype(np.float64) * x.astype(np.float64)
    for v, (h, l) in ((w, (hw, lw)), (x, (hx, lx))):
        assert (np.abs(l) <= 2.0 ** -8 * np.abs(v)).all() and (np.abs(v - h - l) <= 2.0 ** -16 * np.abs(v)).all()
    rel = np.abs(S.one_product(w, x)[0] - exact) / np.abs(exact)
    print("split model against the exact product: largest relative distance %.3e (3 * 2^-16 = %.3e)" % (rel.max(), 3 * 2.0 ** -16))
    assert rel.max() <= 3 * 2.0 ** -16
    assert rel.max() > 3 * 2.0 ** -18


def test_f32_product_holds_the_rounded_fp32_product(sample):
    w, x = sample[:2]
    exp, tol = S.f32_product(w, x)
    assert (np.abs((w * x).astype(np.float64) - exp) <= 0.5 * tol).all()


def _dense_reference(x, w, stride, pad):
    """fp64 convolution by shifted slices: [B,Cout,OH,OW]."""
    B, Cin, H, W = x.shape
    k = w.shape[2]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.zeros((B, Cin, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    out = np.zeros((B, w.shape[0], OH, OW))
    for ky in range(k):
        for kx in range(k):
            out += np.einsum("oc,bchw->bohw", w[:, :, ky, kx].astype(np.float64), xp[:, :, ky:ky + stride * OH:stride, kx:kx + stride * OW:stride])
    return out


@pytest.mark.parametrize("B,Cin,Cout,H,W,stride", S.CONV3X3_SHAPES)
def test_lattice_convolution_covers_every_weight_and_every_output_pixel(B, Cin, Cout, H, W, stride):
    """The builder's own assertions (every (ci, tap) a factor for every co, every output pixel live in some round, no window with two live
    pixels) hold at the GPU test's shapes in a small number of rounds; its expectation is the fp64 convolution of its input to 3 * 2^-16
    (the expectation's indexing is right); image corners and every tap at them are among the live outputs."""
    p = S.LatticeConv(B, Cin, Cout, H, W, stride=stride, seed=Cin + Cout)
    assert 9 <= len(p.rounds) <= S.MAX_ROUNDS and p.tapcov.all() and p.pixcov.all()
    print("3x3 lattice %s: %d rounds" % ((B, Cin, Cout, H, W, stride), len(p.rounds)))
    corner = np.zeros(9, bool)
    for r in range(len(p.rounds)):
        chan, val, sel, _ = p.rounds[r]
        x = p.x(r)
        assert (np.count_nonzero(x, axis=1) == (chan >= 0)).all()               # one live channel per lattice pixel, nothing elsewhere
        lat = np.argwhere(chan[0] >= 0)
        assert (np.diff(np.unique(lat[:, 0])) == 3).all() and (np.diff(np.unique(lat[:, 1])) == 3).all()
        if sel[0, 0, 0] >= 0:
            corner[sel[0, 0, 0] % 9] = True
        if r < 2:
            exp, tol = p.expected(r)
            ref = _dense_reference(x, p.w, stride, 1)
            assert exp.shape == ref.shape and ((exp != 0) == (ref != 0)).all()
            assert (np.abs(exp - ref) <= 3 * 2.0 ** -16 * np.abs(ref)).all()
            assert ((tol > 0) == (exp != 0)).all()
    assert corner[[4, 5, 7, 8]].all() and not corner[[0, 1, 2, 3, 6]].any()     # the top-left output sees exactly the four taps that lie on the map


def test_check_rejects_one_granule_of_one_tap_read_from_the_neighbouring_tap():
    """A stand-in kernel whose weights of channels 8 .. 15 at the centre tap are those of the tap to its right -- one 16-byte granule of
    one weight row per output channel, invisible to a max-norm bound on dense data -- fails the per-output check in the rounds where a
    lattice pixel carries one of those channels; the faithful stand-in, rounded to fp32, passes every round."""
    B, Cin, Cout, H, W, stride = S.CONV3X3_SHAPES[0]
    p = S.LatticeConv(B, Cin, Cout, H, W, stride=stride, seed=1)
    bad = p.w.copy()
    bad[:, 8:16, 1, 1] = p.w[:, 8:16, 1, 2]
    caught = 0
    for r in range(len(p.rounds)):
        sel, xsel = p.rounds[r][2:]
        exp, tol = p.expected(r)
        assert S.check(exp.astype(np.float32), exp, tol) <= 0.5
        touched = (sel >= 0) & (sel % 9 == 4) & (sel // 9 >= 8) & (sel // 9 < 16)
        got = S.select_products(bad.reshape(Cout, -1), sel, xsel)[0].astype(np.float32)
        if touched.any():
            with pytest.raises(AssertionError, match="outside the one-product tolerance"):
                S.check(got, exp, tol)
            caught += 1
        else:
            S.check(got, exp, tol)
    assert caught > 0


def test_dgrad_filter_is_the_input_gradient_of_the_convolution():
    rs = np.random.RandomState(2)
    w, x, go = rs.randn(5, 4, 3, 3), rs.randn(1, 4, 6, 7), rs.randn(1, 5, 6, 7)
    y = _dense_reference(x, w, 1, 1)
    gx = _dense_reference(go, S.dgrad_filter(w), 1, 1)
    assert np.isclose((y * go).sum(), 0.5 * ((y * go).sum() + (gx * x).sum()))   # <conv(x), go> == <x, conv'(go)>: the adjoint
    eps = np.zeros_like(x)
    eps[0, 2, 3, 4] = 1.0
    assert np.isclose((_dense_reference(eps, w, 1, 1) * go).sum(), gx[0, 2, 3, 4])


@pytest.mark.parametrize("B,Cin,Cout,n", S.GEMM_SHAPES + [S.CONV1X1_2D_SHAPE[:3] + (S.CONV1X1_2D_SHAPE[3] * S.CONV1X1_2D_SHAPE[4] // 4,),
                                                           (S.CONV64_SHAPE[0], 64, 64, S.CONV64_SHAPE[1])])
def test_one_hot_gemm_covers_every_weight(B, Cin, Cout, n):
    p = S.OneHotGemm(B, Cin, Cout, n, seed=n)
    x = p.x()
    assert (np.count_nonzero(x, axis=1) == 1).all()
    for b in range(B):
        assert set(np.nonzero(x[b])[0]) == set(range(Cin))                      # every channel live in every image
    exp, tol = p.expected()
    ref = np.einsum("oc,bcn->bon", p.w.astype(np.float64), x.astype(np.float64))
    assert (exp != 0).all() and (tol > 0).all() and (np.abs(exp - ref) <= 3 * 2.0 ** -16 * np.abs(ref)).all()


def test_one_hot_map_leaves_dense_values_where_a_strided_product_must_not_read():
    B, Cin, Cout, H, W = S.CONV1X1_2D_SHAPE
    p = S.OneHotGemm(B, Cin, Cout, (H // 2) * (W // 2), seed=1)
    x = p.x_map(H, W, 2)
    assert np.array_equal(x[:, :, ::2, ::2].reshape(B, Cin, -1), p.x())
    rest = np.ones((H, W), bool)
    rest[::2, ::2] = False
    assert (x[:, :, rest] != 0).all()


@pytest.mark.parametrize("B,Cin,Cout,H,W,taps", [s[:5] + (9,) for s in S.WGRAD3X3_SHAPES] + [S.WGRAD1X1_SHAPE[:3] + (S.WGRAD1X1_SHAPE[3] // 32, 32, 1)])
def test_one_hot_weight_gradient_is_one_product_per_output(B, Cin, Cout, H, W, taps):
    """Every pixel of the contraction hosts a channel, every channel is live at one pixel, and the expectation is the fp64 weight gradient
    (exact zeros where the tap falls off the map, which the 3x3 form must have and the 1x1 form cannot)."""
    p = S.OneHotWgrad(B, Cin, Cout, H, W, taps=taps, seed=Cin + taps)
    x = p.x()
    assert len(np.unique(p.pos)) == B * H * W
    exp, tol = p.expected()
    k = 3 if taps == 9 else 1
    xp = np.zeros((B, Cin, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    ref = np.zeros((Cout, Cin, k, k))
    for ky in range(k):
        for kx in range(k):
            oy, ox = (ky, kx) if k == 3 else (1, 1)
            ref[:, :, ky, kx] = np.einsum("bohw,bchw->oc", p.go.astype(np.float64), xp[:, :, oy:oy + H, ox:ox + W])
    assert ((exp == 0) == (ref == 0)).all() and (np.abs(exp - ref) <= 3 * 2.0 ** -16 * np.abs(ref)).all()
    assert ((tol == 0) == (exp == 0)).all()
    assert (p.nzero > 0) == (taps == 9) and (exp == 0).sum() == p.nzero


def test_stem_lattice_covers_every_weight_before_the_pool_and_every_pooled_output():
    B, C, H, W = S.STEM_SHAPE
    p = S.LatticeStem(B, H, W, seed=5)
    assert C == 3 and 7 <= len(p.rounds) <= S.MAX_ROUNDS and p.tapcov.all() and p.pixcov.all()
    every_output_positive, share_won = p.coverage()
    print("stem lattice: %d rounds; share of the 64 x 147 weight elements that win a pooled output in some round: %.3f" % (len(p.rounds), share_won))
    assert every_output_positive
    for r in range(2):
        x = p.x(r)
        conv = np.maximum(_dense_reference(x, p.w, 2, 3), 0.0)
        ref = S.pool3x3s2(conv, 0.0)
        exp, tol = p.expected(r)
        assert exp.shape == ref.shape == (B, 64, 16, 16)
        assert ((exp == 0) == (ref == 0)).all() and (np.abs(exp - ref) <= 3 * 2.0 ** -16 * np.abs(ref)).all()
        assert (tol[exp > 0] > 0).all()


def test_pool_restatement_equals_torch():
    import torch
    a = np.random.RandomState(0).randn(2, 3, 9, 12)
    want = torch.nn.functional.max_pool2d(torch.from_numpy(a), 3, 2, 1).numpy()
    assert np.array_equal(S.pool3x3s2(a, -np.inf), want)


@pytest.mark.parametrize("prec", [S.MATCH_BF16X3, S.MATCH_F32])
def test_match_rows_round_trip_and_expectation(prec):
    """encode / decode of the 512-byte rows, and the expectation on rows normalised in numpy: the cosine of a one-hot point with a model
    vertex is that vertex's normalised component."""
    B, N, M = S.MATCH_SHAPE
    scene, model = S.match_inputs(B, N, M, seed=3)
    sn = (scene[0] / np.linalg.norm(scene[0], axis=0, keepdims=True)).T.astype(np.float32)
    mn = (model / np.linalg.norm(model, axis=0, keepdims=True)).T.astype(np.float32)
    srows, mrows = S.encode_match_rows(sn, prec), S.encode_match_rows(mn, prec)
    assert srows.size == N * 512 and mrows.size == M * 512
    if prec == S.MATCH_F32:
        assert np.array_equal(S.decode_match_rows(mrows, prec), mn)
    else:
        hi, lo = S.decode_match_rows(mrows, prec)
        assert np.array_equal(hi, S.parts(mn)[0]) and np.array_equal(lo, S.parts(mn)[1])
    exp, tol = S.match_expected(srows, mrows, N, prec)
    ref = sn.astype(np.float64) @ mn.astype(np.float64).T
    assert exp.shape == (N, M) and (tol > 0).all() and (np.abs(exp - ref) <= 3 * 2.0 ** -16 * np.abs(ref)).all()


def test_rescale_exponents():
    e = S.rescale_exponents(256, 4)
    assert e.shape == (256,) and e.min() >= -20 and e.max() <= 20 and len(np.unique(e)) > 20
    assert np.array_equal(e, S.rescale_exponents(256, 4))
