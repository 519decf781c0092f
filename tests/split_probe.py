"""Test infrastructure only: one-product inputs for the split-bf16 MFMA kernels, and the exact value each output must then have.

The kernels replace an fp32 product w * x by three bf16 products, hi_w * hi_x + hi_w * lo_x + lo_w * hi_x, on operands split by
gdm_split2 (restated in numpy by tests/packed_layout.split) and accumulated in fp32.  On dense data an output is a sum of hundreds of
such terms, and a fault in ONE of them (a dropped lo * hi, a weight row of the neighbouring tap, a lo plane paired with the wrong hi)
is a relative 2^-9 of one term: below the rounding noise of the rest.  The builders here choose inputs for which every output is a
SINGLE product, so the accumulation order does not matter and the expected value is exact by construction:

    one_product(w, x) = hh + hl + lh in fp64, tolerance 2 * 2^-23 * (|hh| + |hl| + |lh|)

Each bf16 x bf16 product is exact in fp32 (8 + 8 significand bits), adding it to an accumulator that holds exact zeros is exact, so at
most two of the additions round, in any order; each is given 2^-23 rather than the round-to-nearest 2^-24 because the rounding mode of
the MFMA's internal adder is not documented and may truncate.  The tolerance is derived from that alone, not from any kernel's output.

Used by tests/test_split_probe_cpu.py (the builders' coverage claims, the tolerance against an fp32 emulation, the mutants it must
reject) and tests/test_gpu_split_probe.py (the kernels)."""
import itertools

import numpy as np

import packed_layout as P

U = 2.0 ** -23

# the shapes of tests/test_gpu_split_probe.py, shared with the CPU test of the builders' coverage claims
CONV3X3_SHAPES = [(4, 64, 128, 8, 32, 1), (4, 128, 200, 8, 32, 1), (4, 256, 128, 8, 32, 1), (2, 128, 128, 16, 64, 2)]   # B Cin Cout H W stride
DGRAD_SHAPE = (4, 128, 128, 8, 32)                                                  # B Cin Cout H W of the forward convolution
GEMM_SHAPES = [(1, 64, 128, 96), (2, 128, 200, 256), (1, 256, 576, 512)]            # B Cin Cout n
CONV1X1_2D_SHAPE = (2, 128, 136, 8, 64)                                             # B Cin Cout H W, read at stride 1 and 2
CONV64_SHAPE = (2, 1000)                                                            # B m
# B Cin Cout H W parts.  The contraction of a [1, ., 4, 32] map is ONE 128-pixel chunk, which no two parts divide (ops._wgrad_packed
# refuses it): the K split in two runs on the smallest map that has two chunks, the same one with two images.
WGRAD3X3_SHAPES = [(1, 256, 8, 4, 32, None), (2, 256, 8, 4, 32, 2)]
WGRAD1X1_SHAPE = (1, 256, 8, 128)                                                   # B Cin Cout P: the smallest gemm_wgrad takes
STEM_SHAPE = (1, 3, 64, 64)
MATCH_SHAPE = (1, 256, 333)                                                         # B N M
MAX_ROUNDS = 40


def bf16_to_f64(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def parts(v):
    """fp32 v -> (hi, lo) of gdm_split2 as fp64 arrays of v's shape."""
    hi, lo = P.split(v)
    return bf16_to_f64(hi), bf16_to_f64(lo)


def from_parts(hw, lw, hx, lx):
    """(expected, tolerance) of one split product from the operands' parts (fp64, broadcasting)."""
    hh, hl, lh = hw * hx, hw * lx, lw * hx                # each exact in fp64 (and in fp32); their fp64 sum spans < 53 bits: exact too
    return hh + hl + lh, 2 * U * (np.abs(hh) + np.abs(hl) + np.abs(lh))


def one_product(w, x):
    """(hh + hl + lh in fp64, 2 * 2^-23 * (|hh| + |hl| + |lh|)) for fp32 w, x."""
    return from_parts(*parts(w), *parts(x))


def f32_product(w, x):
    """The fp32-MFMA form (MATCH_F32): the product itself, one fp32 rounding of unknown mode: 2^-23 |w x|."""
    p = np.asarray(w, np.float32).astype(np.float64) * np.asarray(x, np.float32).astype(np.float64)
    return p, U * np.abs(p)


def magnitudes(rs, shape, lo=-6.0, hi=6.0):
    """Dense fp32 values of random sign and magnitude in [2^lo, 2^hi], with random significands."""
    return (rs.choice([-1.0, 1.0], size=shape) * 2.0 ** rs.uniform(lo, hi, size=shape)).astype(np.float32)


def rescale_exponents(C, seed):
    """Integers in [-20, 20], one per channel: channel c is scaled by 2^e(c) and its weights by 2^-e(c)."""
    return np.random.RandomState(seed).randint(-20, 21, size=C)


def check(got, exp, tol, what=""):
    """Every output against its one product: an expected zero must be 0.0, everything else within its tolerance.  Returns the largest
    |got - expected| / tolerance (0 where nothing is expected to be non-zero)."""
    got = np.asarray(got, np.float64)
    assert got.shape == exp.shape == tol.shape, (what, got.shape, exp.shape, tol.shape)
    zero = tol == 0
    assert (exp[zero] == 0).all()
    wrong = zero & (got != 0)
    assert not wrong.any(), "%s: %d outputs that must be exactly zero are not, first at %s = %r" % (
        what, wrong.sum(), tuple(np.argwhere(wrong)[0]), got[wrong][0])
    live = ~zero
    if not live.any():
        return 0.0
    ratio = np.zeros(got.shape)
    ratio[live] = np.abs(got - exp)[live] / tol[live]
    bad = ~(ratio <= 1.0)                                 # (a NaN is bad)
    worst = np.unravel_index(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
    assert not bad.any(), "%s: %d of %d outputs outside the one-product tolerance, largest ratio %.3g at %s (got %r, expected %r); first at %s" % (
        what, bad.sum(), live.sum(), ratio[worst], tuple(int(i) for i in worst), got[worst], exp[worst], tuple(np.argwhere(bad)[0]))
    return float(ratio.max())


def window_hits(chan, k, pad, stride):
    """chan int[B,H,W] (the live channel of a pixel, -1: a zero pixel) -> for every output pixel of a k x k / pad / stride convolution
    the one live pixel of its window: (sel int[B,OH,OW] = chan * k * k + tap, -1: none; iy, ix int[B,OH,OW] its position).  Asserts
    that no window holds two live pixels."""
    B, H, W = chan.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    oy, ox = np.arange(OH)[:, None], np.arange(OW)[None, :]
    sel = np.full((B, OH, OW), -1, np.int64)
    sy, sx = np.zeros((B, OH, OW), np.int64), np.zeros((B, OH, OW), np.int64)
    nhit = np.zeros((B, OH, OW), np.int64)
    for ky in range(k):
        for kx in range(k):
            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
            inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            iyc, ixc = np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)
            c = chan[:, iyc, ixc]
            live = inside[None] & (c >= 0)
            nhit += live
            sel = np.where(live, c * k * k + ky * k + kx, sel)
            sy, sx = np.where(live, iyc[None], sy), np.where(live, ixc[None], sx)
    assert nhit.max() <= 1, "a window holds two live pixels"
    return sel, sy, sx


def select_products(w2, sel, xval):
    """w2 f32[Cout,K] dense; output (b, co, s) is w2[co, sel[b, s]] * xval[b, s] (sel -1: an exact zero) -> (expected, tolerance) f64[B,Cout,*S]."""
    hw, lw = parts(w2)
    live = sel >= 0
    k = np.where(live, sel, 0)
    hx, lx = parts(np.where(live, xval, 0).astype(np.float32))
    return from_parts(np.moveaxis(hw[:, k], 0, 1), np.moveaxis(lw[:, k], 0, 1), hx[:, None], lx[:, None])


class LatticeConv:
    """One-product rounds of a k x k convolution (k = 3 / pad 1 / stride 1 or 2; k = 7 / pad 3 / stride 2 for the stem): dense weights
    w f32[Cout,Cin,k,k]; in round r the activation of image b is zero except on the lattice of pitch k at offset (r (k + 1) + b) mod k^2
    of the k x k cell (k + 1 and k^2 are coprime: k^2 rounds walk every position, k rounds every row and every column), so that a window
    holds at most one live pixel, and each lattice pixel carries one live channel: the lattice pixels of all images and rounds, in
    order, take the channels of a sequence of random permutations of 0 .. Cin - 1 (every channel equally often, at unrelated places; a
    plain counter resonates with the lattice and leaves some (ci, tap) uncovered for ever).  Rounds are added, min_rounds at the least, until every (ci, tap) has been the factor of some output (for every
    co: the weights are dense) and every output pixel of every image has had a live pixel in its window."""

    def __init__(self, B, Cin, Cout, H, W, k=3, stride=1, seed=0, min_rounds=9):
        rs = np.random.RandomState(seed)
        self.B, self.Cin, self.Cout, self.H, self.W, self.k, self.pad, self.stride = B, Cin, Cout, H, W, k, k // 2, stride
        self.w = magnitudes(rs, (Cout, Cin, k, k))
        self.rounds = []
        stream = np.zeros(0, np.int64)
        tapcov = np.zeros((Cin, k * k), bool)
        pixcov = None
        while len(self.rounds) < MAX_ROUNDS:
            r = len(self.rounds)
            chan = np.full((B, H, W), -1, np.int64)
            for b in range(B):
                off = (r * (k + 1) + b) % (k * k)
                ys, xs = np.arange(off // k, H, k), np.arange(off % k, W, k)
                n = len(ys) * len(xs)
                while len(stream) < n:
                    stream = np.concatenate([stream, rs.permutation(Cin)])
                chan[b][np.ix_(ys, xs)] = stream[:n].reshape(len(ys), len(xs))
                stream = stream[n:]
            val = np.where(chan >= 0, magnitudes(rs, (B, H, W)), 0).astype(np.float32)
            sel, sy, sx = window_hits(chan, k, self.pad, stride)
            xsel = val[np.arange(B)[:, None, None], sy, sx]
            live = sel >= 0
            tapcov[sel[live] // (k * k), sel[live] % (k * k)] = True
            pixcov = live if pixcov is None else (pixcov | live)
            self.rounds.append((chan, val, sel, xsel))
            if tapcov.all() and pixcov.all() and r + 1 >= min_rounds:
                break
        self.tapcov, self.pixcov = tapcov, pixcov
        assert tapcov.all(), "%d (ci, tap) pairs are the factor of no output after %d rounds" % ((~tapcov).sum(), len(self.rounds))
        assert pixcov.all(), "%d output pixels are zero in every round" % (~pixcov).sum()

    def x(self, r):
        """f32[B,Cin,H,W] of round r."""
        chan, val = self.rounds[r][:2]
        x = np.zeros((self.B, self.Cin, self.H, self.W), np.float32)
        b, y, xx = np.nonzero(chan >= 0)
        x[b, chan[b, y, xx], y, xx] = val[b, y, xx]
        return x

    def expected(self, r):
        """(expected, tolerance) f64[B,Cout,OH,OW] of round r, before any epilogue."""
        sel, xsel = self.rounds[r][2:]
        return select_products(self.w.reshape(self.Cout, -1), sel, xsel)


def dgrad_filter(w):
    """The filter whose 3x3 / s1 / p1 convolution of grad_out is the input gradient: w'[ci, co, ky, kx] = w[co, ci, 2 - ky, 2 - kx]."""
    return np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


class OneHotGemm:
    """1x1 / GEMM: dense w f32[Cout,Cin]; pixel j of image b (of the n that the product READS) is one-hot in channel (j + b) mod Cin.
    n >= Cin, so every weight element is the factor of some output."""

    def __init__(self, B, Cin, Cout, n, seed=0):
        assert n >= Cin
        rs = np.random.RandomState(seed)
        self.B, self.Cin, self.Cout, self.n = B, Cin, Cout, n
        self.w = magnitudes(rs, (Cout, Cin))
        self.chan = (np.arange(n)[None, :] + np.arange(B)[:, None]) % Cin
        self.val = magnitudes(rs, (B, n))
        cov = np.zeros(Cin, bool)
        cov[self.chan.ravel()] = True
        assert cov.all()

    def x(self):
        x = np.zeros((self.B, self.Cin, self.n), np.float32)
        b, j = np.indices((self.B, self.n))
        x[b, self.chan, j] = self.val
        return x

    def x_map(self, H, W, stride):
        """The same pixels as the ones a stride-`stride` 1x1 convolution reads of an [H, W] map (n = (H / stride) * (W / stride)); every
        pixel it must NOT read is dense in every channel, so a wrong pixel offset is no single product."""
        OH, OW = H // stride, W // stride
        assert OH * OW == self.n
        x = magnitudes(np.random.RandomState(self.n + stride), (self.B, self.Cin, H, W))
        x[:, :, ::stride, ::stride] = self.x().reshape(self.B, self.Cin, OH, OW)
        return x

    def expected(self):
        """(expected, tolerance) f64[B,Cout,n]."""
        return select_products(self.w, self.chan, self.val)


class OneHotWgrad:
    """Weight gradient of a 3x3 / s1 / p1 convolution (taps 9) or of a 1x1 product (taps 1): channel ci of x is one-hot at a single
    pixel r_ci of a single image, grad_out is dense.  dW[co, ci, ky, kx] = go[b_ci, co, r_ci - (ky - 1, kx - 1)] * x[ci, r_ci], an exact
    zero where that pixel is off the map.  With Cin >= B * H * W every pixel of the contraction hosts a channel (the four corners and
    every edge pixel included)."""

    def __init__(self, B, Cin, Cout, H, W, taps=9, seed=0):
        rs = np.random.RandomState(seed)
        self.B, self.Cin, self.Cout, self.H, self.W, self.taps = B, Cin, Cout, H, W, taps
        npix = B * H * W
        self.pos = np.concatenate([rs.permutation(npix) for _ in range(-(-Cin // npix))])[:Cin]
        self.go = magnitudes(rs, (B, Cout, H, W))
        self.val = magnitudes(rs, (Cin,))
        if Cin >= npix:
            assert len(np.unique(self.pos)) == npix

    def x(self):
        x = np.zeros((self.B, self.Cin, self.H * self.W), np.float32)
        x[self.pos // (self.H * self.W), np.arange(self.Cin), self.pos % (self.H * self.W)] = self.val
        assert (np.count_nonzero(x, axis=(0, 2)) == 1).all()
        return x.reshape(self.B, self.Cin, self.H, self.W)

    def expected(self):
        """(expected, tolerance) f64[Cout,Cin,k,k] (k = 3 or 1)."""
        k = 3 if self.taps == 9 else 1
        b, ry, rx = self.pos // (self.H * self.W), self.pos % (self.H * self.W) // self.W, self.pos % self.W
        exp, tol = np.zeros((self.Cout, self.Cin, k, k)), np.zeros((self.Cout, self.Cin, k, k))
        hx, lx = parts(self.val)
        hg, lg = parts(self.go)
        nzero = 0
        for ky in range(k):
            for kx in range(k):
                y, x = ry - ky + k // 2, rx - kx + k // 2
                ok = (y >= 0) & (y < self.H) & (x >= 0) & (x < self.W)
                yc, xc = np.clip(y, 0, self.H - 1), np.clip(x, 0, self.W - 1)
                e, t = from_parts(hg[b, :, yc, xc].T, lg[b, :, yc, xc].T, hx[None], lx[None])       # [Cout, Cin]
                exp[:, :, ky, kx], tol[:, :, ky, kx] = np.where(ok[None], e, 0), np.where(ok[None], t, 0)
                nzero += (~ok).sum()
        self.nzero = nzero * self.Cout
        return exp, tol


def pool_windows(a, fill):
    """The nine members of every 3x3 / stride 2 / pad 1 window of a[..., H, W], as nine [..., PH, PW] views of a copy padded with fill."""
    H, W = a.shape[-2:]
    PH, PW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = np.full(a.shape[:-2] + (2 * PH + 1, 2 * PW + 1), fill, a.dtype)
    p[..., 1:H + 1, 1:W + 1] = a
    return [p[..., dy:dy + 2 * PH:2, dx:dx + 2 * PW:2] for dy in range(3) for dx in range(3)]


def pool3x3s2(a, fill):
    """max over 3x3 / stride 2 / pad 1 windows of a[..., H, W] (padding = fill)."""
    return np.maximum.reduce(pool_windows(a, fill))


class LatticeStem(LatticeConv):
    """The stem: 7x7 / stride 2 / pad 3 on a lattice of pitch 7, scale 1, shift 0; the expected value goes through the kernel's ReLU and
    its 3x3 / stride 2 / pad 1 max-pool, a pooled output getting the largest tolerance of its window."""

    def __init__(self, B, H, W, seed=0):
        super().__init__(B, 3, 64, H, W, k=7, stride=2, seed=seed, min_rounds=7)

    def expected(self, r):
        exp, tol = super().expected(r)
        return pool3x3s2(np.maximum(exp, 0.0), 0.0), pool3x3s2(tol, 0.0)

    def coverage(self):
        """(every (co, pooled pixel) positive in some round?, share of the weight elements that WIN a pooled output in some round)."""
        pos = None
        won = np.zeros((self.Cout, self.Cin * 49), bool)
        for r in range(len(self.rounds)):
            e = LatticeConv.expected(self, r)[0]
            pooled = pool3x3s2(np.maximum(e, 0.0), 0.0)
            pos = pooled > 0 if pos is None else (pos | (pooled > 0))
            for v, s in zip(pool_windows(e, 0.0), pool_windows(self.rounds[r][2], -1)):       # a member wins where it IS the pooled value
                b, co, y, x = np.nonzero((v == pooled) & (pooled > 0))
                won[co, s[b, y, x]] = True
        return bool(pos.all()), float(won.mean())


MATCH_BF16X3, MATCH_F32 = 0, 1


def match_inputs(B, N, M, seed=0):
    """scene f32[B,128,N]: point n one-hot in channel n mod 128; model f32[128,M] dense."""
    rs = np.random.RandomState(seed)
    scene = np.zeros((B, 128, N), np.float32)
    n = np.arange(N)
    scene[:, n % 128, n] = magnitudes(rs, (B, N), -3.0, 3.0)
    assert (np.count_nonzero(scene, axis=1) == 1).all() and N >= 128
    return scene, magnitudes(rs, (128, M), -3.0, 3.0)


def decode_match_rows(rows, precision):
    """The packed rows of gdm_match.hip's header (u8[R * 512]) -> BF16X3: (hi, lo) f64[R,128] from 128 bf16 hi | 128 bf16 lo;
    F32: f32[R,128]."""
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 512)
    if precision == MATCH_F32:
        return rows.view(np.float32).reshape(-1, 128)
    h = rows.view(np.uint16).reshape(-1, 256)
    return bf16_to_f64(h[:, :128]), bf16_to_f64(h[:, 128:])


def encode_match_rows(v, precision):
    """f32[R,128] -> rows in the same format, without the pack kernel's normalisation (both parts of the live channel are then live)."""
    v = np.ascontiguousarray(v, np.float32)
    if precision == MATCH_F32:
        return v.view(np.uint8).reshape(-1).copy()
    hi, lo = P.split(v)
    return np.concatenate([hi, lo], axis=1).view(np.uint8).reshape(-1).copy()


def match_expected(scene_rows, model_rows, N, precision):
    """(expected, tolerance) f64[N,M] of sim for scene rows that are one-hot in channel n mod 128 (asserted), from the decoded operands."""
    c = np.arange(N) % 128
    if precision == MATCH_F32:
        s, m = decode_match_rows(scene_rows, precision), decode_match_rows(model_rows, precision)
        assert (np.count_nonzero(s, axis=1) == 1).all() and (s[np.arange(N), c] != 0).all()
        return f32_product(s[np.arange(N), c][:, None], m[:, c].T)
    (hs, ls), (hm, lm) = decode_match_rows(scene_rows, precision), decode_match_rows(model_rows, precision)
    assert (np.count_nonzero(hs, axis=1) == 1).all() and (hs[np.arange(N), c] != 0).all()
    assert (np.count_nonzero(ls, axis=1) <= 1).all() and (np.count_nonzero(ls, axis=1) == (ls[np.arange(N), c] != 0)).all()
    return from_parts(hs[np.arange(N), c][:, None], ls[np.arange(N), c][:, None], hm[:, c].T, lm[:, c].T)


def emulate_fp32_orders(w, x):
    """The three products added into an fp32 zero in each of the six orders, round to nearest: f64[6, ...]."""
    (hw, lw), (hx, lx) = parts(w), parts(x)
    terms = [(hw * hx).astype(np.float32), (hw * lx).astype(np.float32), (lw * hx).astype(np.float32)]
    out = []
    for order in itertools.permutations(range(3)):
        acc = np.zeros_like(terms[0])
        for i in order:
            acc = (acc + terms[i]).astype(np.float32)
        out.append(acc.astype(np.float64))
    return np.stack(out)
