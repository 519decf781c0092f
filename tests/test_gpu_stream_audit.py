"""The forked step under tests/stream_audit.py: every fork the product has, audited for ordering (R1) and lifetime (R2).

Per program: one un-audited warm-up step inside an ops.BufferPool scope, then, under audited(), TWO consecutive steps with every
static input overwritten in between on the launch stream (what infer.GraphedPipeline.__call__ does with copy_), so that cross-step
write-after-read hazards on inputs and on pool buffers are in the log too.  Shapes are the smallest the step takes: batch 2,
N = 1024 scene points (the pyramid's minimum), M = 1024 model vertices.  Nothing here stages a race on the device: the bad
orderings of the sensitivity checks exist only as edited copies of the recorded log."""
import json
import os

import numpy as np
import pytest
import torch

import stream_audit as sa
from geometric_aware_dense_matching_amd import infer, ops, settings, synthetic
from geometric_aware_dense_matching_amd.config import make_model_cfg

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
B, N, M, S = 2, 1024, 1024, 256
ALL_PARTS = ["mesh", "point", "pyr", "psp"]

# program -> (model, step keywords, SIDE_PARTS, MESH_FORK_LATE, the side-stream roles the log must hold)
PROGRAMS = {
    "ffb6d-default": ("ffb6d", {}, ["mesh", "point", "pyr"], True, {"side0", "side1", "side2"}),
    "ffb6d-all": ("ffb6d", {}, ALL_PARTS, True, {"side0", "side1", "side2", "side3"}),
    "ffb6d-early-mesh": ("ffb6d", {}, ["mesh", "point", "pyr"], False, {"side0", "side1", "side2"}),
    "ffb6d-soft": ("ffb6d", dict(match_gamma=16.0, pose_opts=dict(weights="conf", targets="soft")), ["mesh", "point", "pyr"], True,
                   {"side0", "side1", "side2"}),
    "dgcnn": ("dgcnn", {}, ["mesh", "point", "pyr"], True, {"side0", "side1"}),          # the seg-mask fork (0) and the mesh trunk (1)
    "frames": ("ffb6d", {}, ["mesh", "point", "pyr"], True, {"side0", "side1", "side2"}),
}

# Waits whose removal from the recorded log leaves no violation: the first frames of the site (" < " between them) -> (the programs
# it holds for, None = every program that has the site; the reason).  Also a list of waits the step may not need for its data.
# Checked both ways: a site listed here that does produce a violation fails too.
FFB6D = ("ffb6d-default", "ffb6d-all", "ffb6d-early-mesh", "ffb6d-soft")
REDUNDANT = {
    'ffb6d.py:exchange: self.side.wait_event(ev_image) < ffb6d.py:forward: lanes.exchange(to_point=(inputs["cld_rgb_nrm"],))':
        (None, "the point lane's first kernel also waits for READY_CLOUD, and side stream 2 records that behind its own wait for "
               "the launch stream: what the launch stream wrote into cld_rgb_nrm is ordered through the pyramid fork.  Needed as "
               "soon as `pyr` is not forked."),
    "ops.py:__enter__: self.side.wait_event(self.start) < geoMatch.py:forward: with ops.fork(rgb.device, 1, start=ev0) as f:":
        (None, "the mesh branch reads parameters and buffers only: the wait places the fork in the graph, it orders no data"),
    "ops.py:__enter__: self.side.wait_stream(self.cur) < geoMatch.py:forward: with ops.fork(rgb.device, 1) as f:":
        (None, "the early mesh fork: parameters and buffers only, as above"),
    "ops.py:__enter__: self.side.wait_stream(self.cur) < geoMatch_DGCNN.py:forward: with ops.fork(x.device, 1) as f:":
        (None, "the DGCNN mesh trunk: parameters and buffers only, as above"),
}
# The same for record_stream call sites under R2.
REDUNDANT_KEEP = {
    'ffb6d.py:_keep: t.record_stream(lane) < ffb6d.py:exchange: self._keep(to_point, self.side) < ffb6d.py:forward: lanes.exchange(to_point=(inputs["cld_rgb_nrm"],))':
        (FFB6D, "cld_rgb_nrm is a static input here: it exists before the step and R2 exempts it (in `frames` the front end allocates "
                "it inside the step, and there the call is needed)"),
    "ops.py:use: t.record_stream(self.side) < pyramid.py:build_pyramid: f.use(cld, dpt_xyz)":
        (FFB6D, "static inputs, as above"),
    "pyramid.py:wait_ready: v.record_stream(st) < ffb6d.py:exchange: pyramid.wait_ready(self.inputs, self.side)":
        (None, "wait_ready records EVERY pyramid tensor on the waiting stream, and the point lane calls it twice (the cloud-only wait "
               "and this full one): either call's record_stream alone satisfies R2"),
    "pyramid.py:wait_ready: v.record_stream(st) < ffb6d.py:forward: pyramid.wait_ready(inputs, cloud_only=lanes.two)":
        (None, "the other of the two calls above"),
}


def _listed(table, site, name):
    return any(site.startswith(k) and (progs is None or name in progs) for k, (progs, _why) in table.items())


def _ffb6d():
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(G, "geomatch_state.json")))
    model.load_state_dict(synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0), strict=False)
    return model.cuda().eval()


def _dgcnn():
    from geometric_aware_dense_matching_amd.config import make_dgcnn_cfg
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
    torch.manual_seed(0)
    model = GeoMatchDGCNN(make_dgcnn_cfg(n_mesh_node=M, dataset="ycbv"), 2, model_points=synthetic.make_model_points(2, M, 269.573))
    sd = synthetic.synthetic_state_dict({k: v for k, v in model.state_dict().items() if k != "model_emb.mesh"}, seed=4)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _ffb6d() if kind == "ffb6d" else _dgcnn()
        return made[kind]
    return get


def _launch_stream():
    """A stream that is none of the package's side streams.  torch hands streams out of a pool of 32 per device, round robin: the
    33rd torch.cuda.Stream() of a process IS the first again, so in a long pytest process a new stream can be the very stream
    ops.side_stream(k) holds -- the fork onto k is then no fork, and the log has one role fewer.  All four side streams are made
    first, so that none of them can be created later on top of the stream returned here."""
    dev = torch.device("cuda", torch.cuda.current_device())
    taken = {ops.side_stream(dev, k).cuda_stream for k in range(4)}
    for _ in range(40):
        s = torch.cuda.Stream()
        if s.cuda_stream not in taken:
            return s
    raise AssertionError("no stream outside the side streams in 40 draws")


def _crops(seed, keys):
    batch = synthetic.make_batch(seed=seed, batch=B, n_points=N)
    return {k: torch.from_numpy(batch[k]).cuda() for k in keys}


def _frames(seed):
    rs = np.random.RandomState(seed)
    fr = [synthetic.make_frame(rs) for _ in range(B)]
    det = [synthetic.make_box_mask(rs) for _ in range(B)]
    K = np.stack([synthetic.LM_K * np.float32(1.0 + 0.07 * b) for b in range(B)]).astype(np.float32)
    K[:, 2, 2] = 1.0
    d = dict(rgb_u8=np.stack([f[1] for f in fr]), depth=np.stack([f[0] for f in fr]), K=K, bbox_xyxy=np.stack([d[0] for d in det]),
             mask=np.stack([d[1] for d in det]))
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _program(name, models):
    """(step(static inputs) -> outputs, the static inputs, a second set of inputs to overwrite them with, the model)."""
    kind, kw, _, _, _ = PROGRAMS[name]
    model = models(kind)
    if name == "frames":
        seed = torch.full((1,), 3, dtype=torch.int32, device="cuda")
        static, other = _frames(81), _frames(82)
        static["seed"], other["seed"] = seed, torch.full((1,), 4, dtype=torch.int32, device="cuda")

        def step(d):
            return infer.frame_step(model, {k: v for k, v in d.items() if k != "seed"}, S, N, seed=d["seed"], with_pose=True)
        return step, static, other, model
    keys = ("cld_rgb_nrm",) if kind == "dgcnn" else ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")
    return (lambda d: infer.pipeline_step(model, d, with_pose=True, **kw)), _crops(131, keys), _crops(132, keys), model


def run_audit(name, models):
    """The recorded log of program `name` and its report.  Settings are restored whatever happens."""
    _, _, parts, late, _ = PROGRAMS[name]
    saved = (settings.USE_SIDE_STREAMS, list(settings.SIDE_PARTS), settings.MESH_FORK_LATE)
    step, static, other, model = _program(name, models)
    pool = ops.BufferPool()
    launch = _launch_stream()
    try:
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS, settings.MESH_FORK_LATE = True, list(parts), late
        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.stream(launch), ops.buffer_pool(pool):
            step(static)                                                     # warm-up: derived weights and pool buffers exist
            torch.cuda.synchronize()
            known = sa.collect_tensors(model, pool, static, other)
            with sa.audited(known=known) as tr:
                out1 = step(static)
                for k, buf in static.items():                                # on the launch stream, as GraphedPipeline.__call__
                    buf.copy_(other[k], non_blocking=True)
                out2 = step(static)
        torch.cuda.synchronize()
        del out1, out2
    finally:
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS, settings.MESH_FORK_LATE = saved
    return tr, sa.analyse(tr.log, unresolved=tr.unresolved)


def sensitivity(log, what):
    """{site: number of violations the log has without that call site}"""
    out = {}
    for site in sa.sites(log, what):
        rep = sa.analyse(sa.without(log, what, site))
        out[" < ".join(site) or "<outside the package>"] = len(rep.r1) if what == "wait" else len(rep.r2)
    return out


def summary(name, tr, rep):
    waits, keeps = sensitivity(tr.log, "wait"), sensitivity(tr.log, "keep")
    return dict(program=name, accesses=rep.accesses, streams=sorted(rep.streams), calls=dict(rep.calls),
                ordered=sorted(rep.ordered), wait_sites=len(waits), redundant_waits=sorted(s for s, n in waits.items() if not n),
                keep_sites=len(keeps), redundant_keeps=sorted(s for s, n in keeps.items() if not n),
                exceptions=sorted(map(str, rep.used_exceptions)), unresolved=[u[:4] for u in rep.unresolved],
                violations=[str(v) for v in rep.violations])


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_forked_step_is_ordered(name, models):
    tr, rep = run_audit(name, models)
    info = summary(name, tr, rep)
    print(json.dumps(info, indent=1))
    sides = PROGRAMS[name][4]
    # every pointer of every library call was resolved; R1 and R2 report nothing outside the exception table
    assert not rep.unresolved, rep.unresolved[:5]
    assert not rep.violations, "\n" + str(rep)
    # non-vacuity: a silently disabled fork cannot pass
    assert rep.streams == {"main"} | sides                                    # exactly 1 + (forked parts) stream roles
    for s in sides:
        assert rep.calls[s] >= 1, "no library call on " + s
        assert any(w == s and r != s for w, r in rep.ordered), "nothing written on %s is read elsewhere behind an event" % s
    assert any(w == "main" and r != "main" for w, r in rep.ordered)
    # sensitivity: without any one call site of a wait (of a record_stream) the same log has a violation, or the site is listed
    for what, table in (("wait", REDUNDANT), ("keep", REDUNDANT_KEEP)):
        for site, n in sensitivity(tr.log, what).items():
            assert (n == 0) == _listed(table, site, name), "%s site %r: %d violations without it" % (what, site, n)


def test_captured_forked_step_issues_the_eager_steps_sequence(models):
    """The tracker is host-side only, so it also runs around the capture of the forked GraphedPipeline.  The captured step must log
    the same sequence of (entry or op, stream role, ordering call) as the eager step on the same pool: then the eager audit speaks
    for the graph that is replayed."""
    model = models("ffb6d")
    static = _crops(131, ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz"))
    saved = (settings.USE_SIDE_STREAMS, list(settings.SIDE_PARTS), settings.MESH_FORK_LATE)
    launch = _launch_stream()
    sides = {st.cuda_stream for st in ops._side_streams.values()}
    saved_capture = torch.cuda.graph.default_capture_stream
    try:
        # torch.cuda.graph captures on one stream it makes once per process, out of the same pool of 32 (see _launch_stream): where the
        # history of this process has put it on top of a side stream, the capture would fork onto its own stream.  Give it another.
        if saved_capture is None or saved_capture.cuda_stream in sides:
            torch.cuda.graph.default_capture_stream = _launch_stream()
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS, settings.MESH_FORK_LATE = True, ["mesh", "point", "pyr"], True
        with sa.audited(known=sa.collect_tensors(model, static)) as cap:
            gp = infer.GraphedPipeline(model, static, with_pose=True, forked=True, warmup=2)
        assert gp.form == "forked"
        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.stream(launch), ops.buffer_pool(gp.pools["forked"]):
            with sa.audited(known=sa.collect_tensors(model, gp.pools["forked"], gp.static_in)) as eager:
                gp._step()
        torch.cuda.synchronize()
    finally:
        settings.USE_SIDE_STREAMS, settings.SIDE_PARTS, settings.MESH_FORK_LATE = saved
        torch.cuda.graph.default_capture_stream = saved_capture
    last = max(i for i, e in enumerate(cap.log) if e.kind == "sync" and e.op == "sync_all")      # torch.cuda.graph synchronises, then captures
    captured = cap.log[last + 1:]
    # capture_begin itself fills torch's two RNG-state words on the capture stream (nearest package frame: GraphedPipeline._capture,
    # which opens the capture): they belong to the capture, not to the step
    own = [e for e in captured if e.kind == "access" and e.site[:1] and e.site[0].startswith("infer.py:_capture:")]
    assert all(e.name == "aten::fill_" and e.stream.startswith("main") for e in own) and len(own) <= 2, own
    want, got = sa.sequence(eager.log), sa.sequence([e for e in captured if not any(e is o for o in own)])
    assert len(want) > 100 and {r for _, r in want} == {"main", "side0", "side1", "side2"}
    diff = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), None)
    assert diff is None and len(want) == len(got), (len(want), len(got), diff, want[diff:diff + 3] if diff is not None else None,
                                                     got[diff:diff + 3] if diff is not None else None)
    assert not cap.unresolved and not eager.unresolved
    rep = sa.analyse(captured)
    assert not rep.r1, "\n" + str(rep)
    gp.replay()                                                              # the graph that was captured under the tracker replays
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(gp.static_out[k]).all()) for k in ("rgbd", "seg"))
