"""Every hand-written autograd Function of the package, call by call on the tensors a real training step feeds it, against fp64.

The per-operator tests hold these kernels to 1e-4 .. 1e-6 on synthetic tensors; the whole-step tests see real data but can resolve only
an O(1) error (train-mode BatchNorm with a batch variance near eps amplifies every rounding difference of the layers in front of it).
That ill-conditioning belongs to the network, not to any one operator: here each Function is compared on its OWN recorded inputs --
kNN index lists with repeated neighbours, post-ReLU maps full of exact zeros, channels whose variance is about eps, the layer shapes
and argument combinations of the network itself -- at its sibling test's tolerance (tests/train_replay.py: recorder, restatements,
tolerances; profiles/train_replay.md: the measured errors).

Recorded once per module (B = 2, N = 1024, M = 512, train mode, fixed seeds, every training flag at its default, no process group):
  ffb6d           one forward + backward of train_lm.model_fn_dec on the FFB6D variant
  ffb6d_grouped   the same with the mesh branch on the edge-grouped SplineConv training path
  dgcnn_fused     the DGCNN variant on its fused training path (feature kNN, edge stages without edge tensors)
  dgcnn_modules   the DGCNN variant on its default module path (the edge tensors of ops.edge_feature)
  direct          one small direct call of each Function no step reaches (train_replay.UNREACHED)
"""
import pytest
import torch

import train_replay as tr

gpu = pytest.mark.gpu
B, N, M = 2, 1024, 512
STEPS = ("ffb6d", "ffb6d_grouped", "dgcnn_fused", "dgcnn_modules")


# --------------------------------------------------------------------------------------
# CPU: completeness of the table, the recorder on a toy Function
# --------------------------------------------------------------------------------------
def test_every_function_of_the_package_has_a_restatement_or_is_listed():
    """Table keys == the Function subclasses found by introspection, and the list of unreached Functions names only such classes: a
    Function added to the package later fails here until it has a restatement."""
    found = set(tr.package_functions())
    assert len(found) >= 21
    assert set(tr.TABLE) | set(tr.UNREACHED) == found, (sorted(found - set(tr.TABLE)), sorted(set(tr.TABLE) - found))
    assert set(tr.UNREACHED) <= set(tr.TABLE)                  # a listed class is replayed too
    for name, entry in tr.TABLE.items():
        assert entry.fwd < 1e-3 and entry.bwd < 1e-3 and entry.buf_tol < 1e-3 and all(t < 1e-3 for t in entry.grad_tol.values()), name
        assert "::test_" in entry.sibling, name


class _Toy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, buf, k, w):
        ctx.save_for_backward(x, w)
        ctx.k = k
        buf.add_(1.0)                                          # state updated in place, as a BatchNorm's running statistics
        return x * w * k

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g * w * ctx.k, None, None, (g * x * ctx.k).sum(0, keepdim=True)


def test_recorder_on_a_toy_function_gives_complete_records_and_restores_the_class():
    fwd, bwd = _Toy.__dict__["forward"], _Toy.__dict__["backward"]
    x = torch.arange(6.0).view(2, 3).requires_grad_(True)
    w = torch.full((1, 3), 2.0, requires_grad=True)
    buf = torch.zeros(3)
    sink = []
    with tr.recording([_Toy], sink, "toy"):
        y1 = _Toy.apply(x, buf, 3, w)
        y1.relu_()                                             # an in-place activation after the call does not reach the record
        y2 = _Toy.apply(y1, buf, 0.5, w)
        y2.sum().backward()
    assert _Toy.__dict__["forward"] is fwd and _Toy.__dict__["backward"] is bwd
    assert len(sink) == 2 and all(r.complete and r.cls_name == "_Toy" and r.step == "toy" for r in sink)
    a, b = sink
    assert torch.equal(a.args[0], x.detach()) and a.args[2] == 3 and torch.equal(b.args[0], y1.detach()) and b.args[2] == 0.5
    assert a.needs == (True, False, False, True)
    assert torch.equal(a.args[1], torch.zeros(3)) and torch.equal(a.post[1], torch.ones(3)) and torch.equal(b.post[1], torch.full((3,), 2.0))
    assert torch.equal(a.outputs[0], x.detach() * 6.0) and torch.equal(b.outputs[0], y2.detach())
    assert torch.equal(b.grad_outputs[0], torch.ones(2, 3)) and torch.equal(b.grads[0], torch.ones(2, 3))
    assert b.grads[1] is None and b.grads[2] is None and torch.equal(a.grads[0], x.grad)
    assert torch.equal(a.grads[3] + b.grads[3], w.grad)
    with pytest.raises(RuntimeError):                          # ... and an exception in the body restores the class as well
        with tr.recording([_Toy], [], "toy"):
            raise RuntimeError("body failed")
    assert _Toy.__dict__["forward"] is fwd and _Toy.__dict__["backward"] is bwd
    _Toy.apply(x, buf, 1, w)
    assert len(sink) == 2


def test_comparator_measures():
    want = torch.tensor([1e-3, -2e-3])
    assert tr.rel_err(want * 1.001, want) < 1e-5 < 9e-4 < tr.scale_free_err(want * 1.001, want) < 1.1e-3
    assert tr.scale_free_err(torch.zeros(2), torch.zeros(2)) == 0.0 and tr.rel_err(torch.tensor([float("nan")]), torch.ones(1)) != 0.0


# --------------------------------------------------------------------------------------
# GPU: the recorded steps
# --------------------------------------------------------------------------------------
def _step(model, sink, name, seed=5):
    from geometric_aware_dense_matching_amd import train_lm
    dev = torch.device("cuda", 0)
    ds = train_lm.SyntheticCrops(B, N, M, seed=seed)
    batch = torch.utils.data.default_collate([ds[i] for i in range(B)])
    model.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    with tr.recording(list(tr.package_functions().values()), sink, name):
        out, _ = train_lm.model_fn_dec(model, batch, dev)
        out["loss"].backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"].detach()))


def _ffb6d(grouped):
    from geometric_aware_dense_matching_amd import synthetic
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    torch.manual_seed(0)
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M)).cuda().train()
    if grouped:
        model.model_emb.train_path = "grouped"
    return model


def _dgcnn(path):
    from geometric_aware_dense_matching_amd import synthetic
    from geometric_aware_dense_matching_amd.config import make_dgcnn_cfg
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    torch.manual_seed(0)
    model = GeoMatchDGCNN(make_dgcnn_cfg(n_mesh_node=M, dataset="ycbv"), 2, model_points=synthetic.make_model_points(2, M, 269.573))
    model.model_emb.k = 20
    model.train_path = path
    return model.cuda().train()


def _direct_calls(sink):
    """One small call of each Function in train_replay.UNREACHED: repeated neighbours, rows without a model vertex, invisible vertices."""
    from geometric_aware_dense_matching_amd import ops, pointops
    g = torch.Generator().manual_seed(11)
    with tr.recording(list(tr.package_functions().values()), sink, "direct"):
        feat = torch.randn(2, 5, 40, generator=g).cuda().requires_grad_(True)
        idx = torch.randint(0, 40, (2, 70, 3), generator=g)
        idx[:, ::7, 1] = idx[:, ::7, 0]
        w = torch.rand(2, 70, 3, generator=g) + 0.1
        out = pointops.interpolation(feat, idx.int().cuda(), (w / w.sum(2, keepdim=True)).cuda())
        (out * torch.randn(2, 5, 70, generator=g).cuda()).sum().backward()

        R, Mv = 300, 130
        xyz = ((torch.rand(Mv, 3, generator=g) - 0.5) * 0.1).cuda()
        vis = (torch.rand(2, Mv, generator=g) < 0.6).to(torch.uint8).cuda()
        match = torch.randint(0, Mv + 1, (R,), generator=g).int().cuda()
        item = torch.sort(torch.randint(0, 2, (R,), generator=g)).values.int().cuda()
        x = torch.nn.functional.normalize(torch.randn(R, 128, generator=g), dim=1).cuda()
        y = torch.nn.functional.normalize(torch.randn(Mv + 1, 128, generator=g), dim=1).cuda()
        sim = (x @ y.t()).requires_grad_(True)
        loss = ops.circle_rows(sim, match, item, xyz, vis, 0.02)
        (loss * torch.rand(R, generator=g).cuda()).sum().backward()

        for s_, oh, ow in ((3, 32, 32), (5, 17, 23)):                           # a PSP prior, and an odd target size
            src = torch.randn(2, 7, s_, s_, generator=g).cuda().requires_grad_(True)
            (ops.upsample_bilinear(src, (oh, ow)) * torch.randn(2, 7, oh, ow, generator=g).cuda()).sum().backward()
    torch.cuda.synchronize()


def record_steps():
    """-> list of every Record of the four steps and the direct calls."""
    sink = []
    for grouped in (False, True):
        model = _ffb6d(grouped)
        first = len(sink)
        _step(model, sink, "ffb6d_grouped" if grouped else "ffb6d")
        _, src, attr = model.model_emb._csr
        for rec in sink[first:]:
            if rec.cls_name == "_SplineGroupedTrain":
                rec.context.update(src=src, attr=attr)
        del model
    for path in ("fused", "modules"):
        model = _dgcnn(path)
        _step(model, sink, "dgcnn_" + path)
        del model
    _direct_calls(sink)
    return sink


@pytest.fixture(scope="module")
def records():
    sink = record_steps()
    by_class = {}
    for rec in sink:
        by_class.setdefault(rec.cls_name, []).append(rec)
    yield by_class
    for rec in sink:
        rec.__dict__.clear()
    sink.clear()
    by_class.clear()
    torch.cuda.empty_cache()


@gpu
def test_every_function_is_recorded_and_the_unreached_list_is_exact(records):
    counts = {name: {s: sum(r.step == s for r in records.get(name, ())) for s in STEPS + ("direct",)} for name in tr.TABLE}
    for name in sorted(counts):
        print("%-20s %s" % (name, "  ".join("%s %d" % kv for kv in counts[name].items())))
    for name, c in counts.items():
        in_steps = sum(c[s] for s in STEPS)
        if name in tr.UNREACHED:
            assert in_steps == 0 and c["direct"] >= 1, (name, c)              # a class a step reaches comes off the list
        else:
            assert in_steps >= 1, (name, c)
    assert counts["_SplineGroupedTrain"]["ffb6d_grouped"] == 2 and counts["_SplineDirectTrain"]["ffb6d_grouped"] == 1
    assert counts["_SplineAggregate"]["ffb6d"] == 3 and counts["_EdgeBlockTrain"]["dgcnn_fused"] == 6
    assert counts["_EdgeFeature"]["dgcnn_modules"] == 6


@gpu
@pytest.mark.parametrize("name", sorted(tr.TABLE))
def test_recorded_calls_against_fp64(records, name):
    """Every recorded call of the class: outputs, every returned gradient and the buffers it updates in place against the fp64 restatement,
    in both error measures at the class's tolerance; None / shape / dtype of what the backward returned."""
    recs = records.get(name, [])
    assert recs, "no recorded call of %s" % name
    bad, worst, ties, fragile = [], {}, 0, 0
    for k, rec in enumerate(recs):
        # a call none of whose inputs needs a gradient (the first edge tensor, built from the input cloud) is compared forward only
        assert rec.complete or not any(rec.needs), "%s call %d of step %s never saw its backward" % (name, k, rec.step)
        ref = tr.reference(rec)
        ties += ref.info.get("ties", 0)
        fragile += ref.info.get("fragile", 0)
        for what, e1, e2, tol in tr.errors(rec, ref):
            kind = "fwd" if what.startswith("out") else "bwd" if what.startswith("grad") else "buf"
            w = worst.setdefault((rec.step, kind), [0.0, 0.0])
            w[0], w[1] = max(w[0], e1), max(w[1], e2)
        where = "%s call %d (%s)" % (rec.step, k, ", ".join(str(tuple(a.shape)) for a in rec.args if torch.is_tensor(a)))
        bad += ["%s: %s" % (where, f) for f in tr.structure_failures(rec, ref) + tr.failures(rec, ref)]
    for (step, kind), (e1, e2) in sorted(worst.items()):
        print("REPLAY %-20s %-14s %s  calls %3d  max error %.3e  scale-free %.3e" % (name, step, kind, sum(r.step == step for r in recs), e1, e2))
    print("REPLAY %-20s ties between distinct sources %d, fragile pre-activations %d" % (name, ties, fragile))
    assert not bad, "\n".join(bad)


@gpu
@pytest.mark.parametrize("name", sorted(tr.TABLE))
def test_comparator_rejects_a_gradient_off_by_one_part_in_a_thousand(records, name):
    """On the recorded data alone (no kernel runs): one returned gradient of the class times (1 + 1e-3) is rejected, and for the
    gather a gradient that lacks one neighbour slot's contribution.  This is why no tolerance may reach 1e-3."""
    rec = next(r for r in records[name] if r.complete)
    ref = tr.reference(rec)
    i = next(i for i, g in enumerate(ref.grads) if g is not None and rec.grads[i] is not None and float(g.abs().max()) > 0.0
             and i not in tr.TABLE[name].usual_only)
    grads = list(rec.grads)
    grads[i] = rec.grads[i] * (1.0 + 1e-3)
    assert any(f.startswith("grad%d:" % i) for f in tr.failures(rec, ref, grads=grads)), name
    if name in tr.GATHER_ARGS:
        rec = next(r for r in records[name] if r.args[1].shape[2] > 1)
        assert any(f.startswith("grad0:") for f in tr.failures(rec, tr.reference(rec), grads=tr.drop_one_neighbour(rec))), name
