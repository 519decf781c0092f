"""CPU: the soft-assignment training losses without a device -- loss.soft_coord_reference against matching.match_soft_numpy, the
analytic gradient of include/gdm.h against autograd, loss.SoftAssignLoss against a per-item Python loop (soft_coord_cases.loop_loss),
the registration of the operator (no autograd.Function subclass), the LDS / packed-fp32 hazard scan of the new translation unit, the
host-side argument checks and the command-line flags."""
import ctypes
import importlib.util
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import soft_coord_cases as sc
from geometric_aware_dense_matching_amd import loss, matching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t64(*arrays):
    return [torch.from_numpy(np.asarray(a)).double() for a in arrays]


@pytest.mark.parametrize("gamma", [1.0, 16.0, 40.0])
def test_reference_equals_match_soft_numpy(gamma):
    """(1) soft_coord_reference in fp64 on unit rows = match_soft_numpy's lse and soft_xyz to 1e-12."""
    x, y, xyz, _, _ = sc.make_case(33, 50, seed=2, family="copy")
    x64, y64, xyz64 = _t64(x, y, xyz)
    x64, y64 = x64 / x64.norm(dim=1, keepdim=True), y64 / y64.norm(dim=1, keepdim=True)
    lse, soft = loss.soft_coord_reference(x64, y64, xyz64, gamma)
    want = matching.match_soft_numpy(x64.numpy(), y64.numpy().T, xyz64.numpy(), gamma)
    assert np.abs(lse.numpy() - want["lse"]).max() <= 1e-12
    assert np.abs(soft.numpy() - want["soft_xyz"]).max() <= 1e-12


@pytest.mark.parametrize("gamma", [1.0, 16.0, 40.0])
def test_analytic_gradient_equals_autograd(gamma):
    """(2) R = 7, M = 13: G, gx, gy of the header's formulas = torch autograd of the reference in fp64 to 1e-12."""
    x, y, xyz, a, b = sc.make_case(7, 13, seed=3)
    x64, y64, xyz64, a64, b64 = _t64(x, y, xyz, a, b)
    x64.requires_grad_(True)
    y64.requires_grad_(True)
    s = (x64 @ y64.t()).detach().requires_grad_(True)
    logits = gamma * s
    lse_s = torch.logsumexp(logits, dim=1)
    soft_s = torch.exp(logits - lse_s[:, None]) @ xyz64
    ((lse_s * a64).sum() + (soft_s * b64).sum()).backward()
    lse, soft = loss.soft_coord_reference(x64, y64, xyz64, gamma)
    ((lse * a64).sum() + (soft * b64).sum()).backward()
    want = sc.analytic(x64.detach(), y64.detach(), xyz64, a64, b64, gamma)
    assert (want["G"] - s.grad).abs().max().item() <= 1e-12
    assert (want["gx"] - x64.grad).abs().max().item() <= 1e-12
    assert (want["gy"] - y64.grad).abs().max().item() <= 1e-12


def _loss_inputs(B=3, N=40, M=24, seed=5):
    rs = np.random.RandomState(seed)
    labels = (rs.rand(B, N) < 0.5).astype(np.int64)
    labels[1] = 0
    labels[1, :2] = 1                                            # 2 selected points: the item is skipped
    match = rs.randint(0, M + 1, size=(B, N)).astype(np.int64)
    match[0, np.nonzero(labels[0])[0][:3]] = M                   # selected rows without a vertex: weightless, still counted
    f = torch.from_numpy(rs.randn(B, 16, N))
    m = torch.from_numpy(rs.randn(16, M))
    xyz = torch.from_numpy(rs.uniform(-0.1, 0.1, (M, 3)))
    q = np.stack([np.linalg.qr(rs.randn(3, 3))[0] for _ in range(B)])
    RT = torch.from_numpy(np.concatenate([q, rs.randn(B, 3, 1) * 0.3], axis=2))
    cld = torch.from_numpy(rs.randn(B, 9, N) * 0.1)
    return torch.from_numpy(labels), torch.from_numpy(match), f, m, xyz, RT, cld


def _via_module(f, m, xyz, labels, match, x, static, sym_idx=None, weights=(1.0, 1.0), gamma=16.0, beta=0.005):
    """The selection of pointwise_feature_matching (compacted or static all-rows form), then loss.soft_assign_terms in fp64."""
    B, D, N = f.shape
    M = m.shape[1]
    sel = labels == 1
    counts = sel.sum(1)
    sel = sel & (counts >= 3).unsqueeze(1)
    if static:
        bi, pi = torch.arange(B).repeat_interleave(N), torch.arange(N).repeat(B)
    else:
        bi, pi = torch.nonzero(sel, as_tuple=True)
    rows = torch.nn.functional.normalize(f.transpose(1, 2)[bi, pi], dim=1)
    mesh_rows = torch.nn.functional.normalize(m, dim=0).t().contiguous()
    c1 = match[bi, pi]
    c2 = match[bi, sym_idx[pi]] if sym_idx is not None else None
    model = SimpleNamespace(soft_gamma=gamma, soft_beta=beta, soft_xyz_weight=weights[0], soft_nll_weight=weights[1], soft_match="reference")
    return loss.soft_assign_terms(model, rows, mesh_rows, xyz, c1, c2, bi, pi, counts, x, static_shape=(B, N) if static else None,
                                  row_weight=sel.reshape(-1) if static else None)


@pytest.mark.parametrize("static", [False, True])
@pytest.mark.parametrize("target", ["RT", "vertex"])
def test_soft_assign_loss_equals_the_per_item_loop(static, target):
    """(3) fp64, B = 3 with one item of 2 selected points and rows with match_idx == M: both terms and their gradients against the
    Python loop, with the RT target and with the vertex target, compacted and static all-rows form."""
    labels, match, f0, m0, xyz, RT, cld = _loss_inputs()
    x = dict(RT=RT, cld_rgb_nrm=cld) if target == "RT" else {}
    res = []
    for fn in ("module", "loop"):
        f, m = f0.clone().requires_grad_(True), m0.clone().requires_grad_(True)
        if fn == "module":
            lx, ln = _via_module(f, m, xyz, labels, match, x, static)
        else:
            lx, ln = sc.loop_loss(f, m, xyz, labels, match, 16.0, 0.005, RT=RT if target == "RT" else None, cld=cld[:, :3])
        (lx + 0.01 * ln).backward()
        res.append((float(lx.detach()), float(ln.detach()), f.grad.clone(), m.grad.clone()))
    (lx0, ln0, gf0, gm0), (lx1, ln1, gf1, gm1) = res
    assert lx1 > 0 and ln1 > 0
    assert abs(lx0 - lx1) <= 1e-12 and abs(ln0 - ln1) <= 1e-12
    assert (gf0 - gf1).abs().max().item() <= 1e-12 and (gm0 - gm1).abs().max().item() <= 1e-12
    assert gf0[1].abs().max().item() == 0                        # the skipped item gets no gradient
    none = (match == 24) & (labels == 1)
    assert none[0].sum() >= 3 and gf0.transpose(1, 2)[none].abs().max().item() == 0      # weightless rows


def test_symmetric_likelihood_and_the_refused_coordinate_term():
    """(3) symmetric objects: lse - logaddexp of the two columns against the loop; the coordinate term raises ValueError."""
    labels, match, f0, m0, xyz, RT, cld = _loss_inputs(N=24, M=24, seed=6)
    sym = torch.from_numpy(np.random.RandomState(7).permutation(24))
    res = []
    for fn in ("module", "loop"):
        f, m = f0.clone().requires_grad_(True), m0.clone().requires_grad_(True)
        if fn == "module":
            lx, ln = _via_module(f, m, xyz, labels, match, {}, False, sym_idx=sym, weights=(0.0, 1.0))
            assert float(lx) == 0.0                              # a term with weight 0 is not computed
        else:
            _, ln = sc.loop_loss(f, m, xyz, labels, match, 16.0, 0.005, sym_idx=sym, want=("nll",))
        ln.backward()
        res.append((float(ln.detach()), f.grad.clone(), m.grad.clone()))
    assert res[1][0] > 0 and abs(res[0][0] - res[1][0]) <= 1e-12
    assert (res[0][1] - res[1][1]).abs().max().item() <= 1e-12 and (res[0][2] - res[1][2]).abs().max().item() <= 1e-12
    with pytest.raises(ValueError, match="symmetric"):
        _via_module(f0, m0, xyz, labels, match, {}, False, sym_idx=sym, weights=(1.0, 1.0))
    with pytest.raises(ValueError, match="match must be"):
        loss.SoftAssignLoss(match="eager")


def test_the_operator_adds_no_autograd_function_class():
    """(4) the operator is a torch.library custom_op with register_autograd: the package has no Function subclass beyond those
    tests/train_replay.py restates or lists, and both operators exist under the gdm namespace."""
    import train_replay as tr
    from geometric_aware_dense_matching_amd import ops
    found = tr.package_functions()
    assert not [n for n in found if "soft" in n.lower()], sorted(found)
    assert set(found) <= set(tr.TABLE) | set(tr.UNREACHED), sorted(set(found) - set(tr.TABLE) - set(tr.UNREACHED))
    assert not isinstance(ops._soft_coord_fwd, type) and hasattr(torch.ops.gdm, "soft_coord_fwd") and hasattr(torch.ops.gdm, "soft_coord_bwd")


def test_new_kernels_have_no_exposed_packed_fp32_consumer(tmp_path):
    """(5) hipcc -S of gdm_softcoord.hip with the Makefile's flags, then tools/scan_lds_pk_hazard.py: 0 exposed consumers in the three
    instances of soft_coord_kernel and in the partial-sum kernel."""
    csrc = os.path.join(ROOT, "geometric_aware_dense_matching_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, flags=re.M))
    assert "gdm_softcoord.hip" in var["SRCS"].split()
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split()
    hipcc = os.environ.get("HIPCC", var["HIPCC"])
    asm = str(tmp_path / "gdm_softcoord.s")
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, "gdm_softcoord.hip"), "-o", asm], check=True,
                   capture_output=True, timeout=900)
    spec = importlib.util.spec_from_file_location("scan_lds_pk_hazard", os.path.join(ROOT, "tools", "scan_lds_pk_hazard.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    text = open(asm).read()
    kernels = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)))
    assert len([k for k in kernels if "soft_coord_kernel" in k]) == 3 and len(kernels) == 4, kernels
    assert "ds_read" in text and "v_mfma_f32_32x32x16_bf16" in text     # the scan had LDS reads to look at; the matrix cores are used
    assert tool.scan(asm) == {}


def test_entries_refuse_bad_gamma_without_a_device():
    """gamma in {0, -1, 40.5, NaN, inf} comes back as GDM_EINVAL with a message before any HIP call (host pointers, no GPU); so do
    the Python operator's checks, before any launch."""
    from geometric_aware_dense_matching_amd import _lib, ops
    lib = _lib.lib()
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    for gamma in (0.0, -1.0, 40.5, float("nan"), float("inf")):
        assert lib.gdm_soft_coord_fwd_hip(p, p, p, p, p, 5, 7, gamma, p, p, None) == -1, gamma
        assert b"gamma" in lib.gdm_last_error()
        assert lib.gdm_soft_coord_bwd_hip(p, p, p, p, p, 5, 7, gamma, p, p, p, p, p, None) == -1, gamma
        assert b"gamma" in lib.gdm_last_error()
        with pytest.raises(ValueError, match="gamma"):
            ops.soft_coord_match(torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(2, 3), gamma)
    assert lib.gdm_soft_coord_bwd_parts(0, 5) == 0 and lib.gdm_soft_coord_bwd_parts(64, 4096) == 2
    assert lib.gdm_soft_coord_bwd_parts(49152, 4096) == 24
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.soft_coord_match(torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(2, 3), 16.0)


def test_cli_flags_parse_and_zero_weights_leave_the_defaults():
    """(6) --soft-gamma / --soft-xyz-weight / --soft-nll-weight parse in both entry points; weights of 0 leave the model's
    attributes at the class defaults, a non-zero weight sets all three."""
    from geometric_aware_dense_matching_amd import train_lm, train_ycb
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    for mod in (train_lm, train_ycb):
        a = mod.build_parser().parse_args([])
        assert (a.soft_gamma, a.soft_xyz_weight, a.soft_nll_weight) == (16.0, 0.0, 0.0)
        a = mod.build_parser().parse_args(["--soft-gamma", "8", "--soft-xyz-weight", "2.5", "--soft-nll-weight", "0.1"])
        assert (a.soft_gamma, a.soft_xyz_weight, a.soft_nll_weight) == (8.0, 2.5, 0.1)
    for cls in (GeoMatch, GeoMatchDGCNN):
        assert (cls.soft_gamma, cls.soft_beta, cls.soft_xyz_weight, cls.soft_nll_weight) == (16.0, 0.005, 0.0, 0.0)
    off = SimpleNamespace()
    train_lm._set_soft_losses(off, train_lm.build_parser().parse_args(["--soft-gamma", "8"]))
    assert not vars(off)                                         # both weights 0: nothing is set, the class defaults hold
    on = SimpleNamespace()
    train_lm._set_soft_losses(on, train_lm.build_parser().parse_args(["--soft-gamma", "8", "--soft-nll-weight", "0.1"]))
    assert vars(on) == dict(soft_gamma=8.0, soft_xyz_weight=0.0, soft_nll_weight=0.1)
