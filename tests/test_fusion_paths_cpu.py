"""Which form each of the seven point-to-pixel fusion sites of FFB6DEmb takes, and what follows from it, as ONE decision per site:
ffb6d._p2r_path for the fusions (read by the point-term producer, _p2r_fuse, _fused_final_stage and _sparse_final_ok) and
PSPUpsample._eval_path for the up-sampling stages (read by forward and reads_packed_only).  CPU only: the decisions are pure functions
of the layers, the shapes and `settings`; `fused` (fused_eval of the forward, false on a CPU tensor) is passed as true.  The table is
the one the separate, hand-kept copies of these conditions gave before they became one function."""
import contextlib

import pytest
import torch
import torch.nn as nn

from geometric_aware_dense_matching_amd import ffb6d, settings, synthetic
from geometric_aware_dense_matching_amd.config import make_model_cfg
from geometric_aware_dense_matching_amd.ffb6d import FMA64, GEMM, MFMA64, MODULES
from geometric_aware_dense_matching_amd.geoMatch import GeoMatch

DS = [(64, 64, 64), (128, 32, 32), (512, 32, 32), (1024, 32, 32)]        # (C, H, W) of the map each fusion site reads
UP = [(256, 64, 64), (64, 128, 128), (64, 128, 128)]
BATCHES = (1, 2, 16)


@pytest.fixture(scope="module")
def emb():
    M = 8192
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=2048), 1, model_points=synthetic.make_model_points(1, M))
    return model.pcd_emb.eval()


@contextlib.contextmanager
def switches(**kw):
    saved = {k: getattr(settings, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(settings, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(settings, k, v)


def table(emb, B, fused=True):
    """Every decision of one forward at batch B, in the order forward() takes them."""
    n_up = len(emb.rndla_up_stages)
    ds = [ffb6d._p2r_path(emb.ds_fuse_p2r_fuse_layers[i], DS[i][0], fused) for i in range(4)]
    up = [ffb6d._p2r_path(emb.up_fuse_p2r_fuse_layers[i], UP[i][0], fused) for i in range(3)]
    sparse = emb._sparse_final_ok(up[n_up - 2], B)
    pm = [sparse and i == n_up - 2 for i in range(3)]
    packed_only = ([i == 3 and emb._packed_only_consumer(emb.cnn_up_stages[0], (B,) + DS[i]) for i in range(4)]
                   + [i + 1 < n_up - 1 and emb._packed_only_consumer(emb.cnn_up_stages[i + 1], (B,) + UP[i]) for i in range(3)])
    final = [emb._fused_final_stage(i, up[i], B, pm[i]) is not None for i in range(3)]
    return dict(ds=ds, up=up, point_major=[p.point_major for p in ds + up], packed_only=packed_only, final=final, sparse=sparse, pm=pm)


DEFAULT = dict(ds=[MFMA64, GEMM, GEMM, GEMM], up=[GEMM, MFMA64, MFMA64],
               point_major=[True, False, False, False, False, True, True],
               packed_only=[False, False, False, True, True, False, False],
               final=[False, True, False], sparse=True, pm=[False, False, True])


@pytest.mark.parametrize("B", BATCHES)
def test_default_switches(emb, B):
    with torch.no_grad():
        assert table(emb, B) == DEFAULT


@pytest.mark.parametrize("B", BATCHES)
def test_without_the_mfma_gemm(emb, B):
    with torch.no_grad(), switches(USE_MFMA_GEMM=False):
        assert table(emb, B) == dict(ds=[FMA64, GEMM, GEMM, GEMM], up=[GEMM, FMA64, FMA64], point_major=[False] * 7,
                                     packed_only=[False] * 7, final=[False] * 3, sparse=True, pm=[False, False, True])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("off", ["USE_FUSED_UPCONV", "USE_SPARSE_FINAL"])
def test_without_the_sparse_final(emb, B, off):
    with torch.no_grad(), switches(**{off: False}):
        assert table(emb, B) == dict(DEFAULT, sparse=False, pm=[False] * 3)


@pytest.mark.parametrize("B", BATCHES)
def test_reads_packed_only(emb, B):
    up_1, up_2, up_3 = emb.cnn_up_stages[0][0], emb.cnn_up_stages[1][0], emb.cnn_up_stages[3][0]
    a, b, c = (B, 1024, 32, 32), (B, 256, 64, 64), (B, 64, 128, 128)
    with torch.no_grad():
        assert [up_1.reads_packed_only(s) for s in (a, b, c)] == [True, False, False]
        assert [up_2.reads_packed_only(s) for s in (a, b, c)] == [False, True, False]
        assert [up_3.reads_packed_only(s) for s in (a, b, c)] == [False, False, False]
        assert not up_1.reads_packed_only((B, 1024, 32, 24))
        with switches(USE_MFMA_GEMM=False):
            assert not any(u.reads_packed_only(s) for u in (up_1, up_2, up_3) for s in (a, b, c))


@pytest.mark.parametrize("site", range(7))
def test_an_unknown_activation_sends_the_site_to_the_modules(emb, site):
    layers = list(emb.ds_fuse_p2r_fuse_layers) + list(emb.up_fuse_p2r_fuse_layers)
    pres = list(emb.ds_fuse_p2r_pre_layers) + list(emb.up_fuse_p2r_pre_layers)
    fuse, c = layers[site], (DS + UP)[site][0]
    saved = fuse.activation
    try:
        fuse.activation = nn.Tanh()
        with torch.no_grad():
            t = table(emb, 2)
            assert (t["ds"] + t["up"])[site] is MODULES
            assert [p for i, p in enumerate(t["ds"] + t["up"]) if i != site] == [p for i, p in enumerate(DEFAULT["ds"] + DEFAULT["up"]) if i != site]
            assert t["sparse"] == (site != 6) and t["final"][1] == (site != 5)
            x, p = torch.zeros(1, c, 2, 2), torch.zeros(1, pres[site].conv.in_channels, 3, 1)
            assert emb._p2r_point_term(MODULES, pres[site], fuse, None, p) is None
            with pytest.raises(RuntimeError):
                emb._p2r_fuse(MODULES, pres[site], fuse, None, x, p, None, torch.zeros(1, 4, 1, dtype=torch.int32), pixel_major=True)
    finally:
        fuse.activation = saved


def test_training_and_autograd_take_the_modules_everywhere(emb):
    ups = [emb.cnn_up_stages[0][0], emb.cnn_up_stages[1][0], emb.cnn_up_stages[3][0]]
    shapes = [(2, 1024, 32, 32), (2, 256, 64, 64), (2, 64, 128, 128)]
    # the forward passes fused_eval(inputs["rgb"], self), which is false in either state, whatever the device
    assert torch.is_grad_enabled() and not ffb6d.fused_eval(torch.zeros(1), emb)
    assert not any(u.reads_packed_only(s) for u in ups for s in shapes)           # eval, autograd on
    emb.train()
    try:
        with torch.no_grad():
            assert not ffb6d.fused_eval(torch.zeros(1), emb)
            t = table(emb, 2, fused=False)
            assert not any(u.reads_packed_only(s) for u in ups for s in shapes)   # training, autograd off
    finally:
        emb.eval()
    assert t["ds"] + t["up"] == [MODULES] * 7 and t["point_major"] == [None] * 7
    assert not any(t["packed_only"]) and not any(t["final"]) and not t["sparse"] and not any(t["pm"])


@pytest.mark.parametrize("site,path", [(0, MFMA64), (0, FMA64), (1, GEMM), (4, GEMM), (5, MFMA64), (5, FMA64)])
def test_the_point_term_has_the_layout_its_path_reads(emb, site, path):
    """path.point_major is the one attribute both sides read: _p2r_point_term writes [B, n', C] where it is true and [B, C, n'] where
    it is false (checked here on the library-GEMM forms, which run on the CPU), and the MFMA64 executor hands it to its kernel as
    t_point_major; the FMA64 and GEMM kernels take channel-major terms only."""
    pre = (list(emb.ds_fuse_p2r_pre_layers) + list(emb.up_fuse_p2r_pre_layers))[site]
    fuse = (list(emb.ds_fuse_p2r_fuse_layers) + list(emb.up_fuse_p2r_fuse_layers))[site]
    c, n = (DS + UP)[site][0], 5
    p = torch.randn(2, pre.conv.in_channels, n, 1, generator=torch.Generator().manual_seed(site))
    with torch.no_grad(), switches(USE_POINTWISE=False):
        t = emb._p2r_point_term(path, pre, fuse, emb._split_fuse_weight(fuse, c), p)
        wb = fuse.conv.weight.view(c, 2 * c)[:, c:]
        want = torch.einsum("oc,bcn->bon", wb.double(), pre(p).reshape(2, c, n).double())
    assert t.shape == ((2, n, c) if path.point_major else (2, c, n))
    assert torch.allclose((t.transpose(1, 2) if path.point_major else t).double(), want, rtol=1e-5, atol=1e-5)
    assert (MFMA64.point_major, FMA64.point_major, GEMM.point_major, MODULES.point_major) == (True, False, False, None)
