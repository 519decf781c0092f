"""Inference drivers: the multi-object `test()` loop and the whole step as one hipGraph launch.

The reference's `test()` keeps one GeoMatch per object id and runs every detected instance as its own batch-1
forward (`cal_result_multimodel`, /root/reference/train_lm.py:298-314), recomputing the whole mesh branch per instance.
Here instances are grouped by object and each group is ONE batched pass (neighbour pyramid, forward, matching, pose);
results come back in the original instance order with the reference's concatenated layout
(`seg [bs,2,N]`, `rgbd [bs,128,N]`, `mesh [bs,128,M]`)."""
import torch

from . import frontend, matching, ops, pose, pyramid, settings

_PREC = {"bf16x3": ops.MATCH_BF16X3, "f32": ops.MATCH_F32, 0: 0, 1: 1}


def _plane_normals(model, pose_opts):
    """The model's unit normals when pose_opts asks for point-to-plane ICP (cached on the mesh branch: normalised once per model)."""
    return model.model_emb.unit_normals() if (pose_opts or {}).get("icp_metric") == "plane" else None


def _twoway(match_twoway, pose_opts, match_gamma, match_dual=False):
    """The two-way kernel is taken when asked for, and when pose_opts' pair_filter needs its col_idx; not together with soft matching.
    match_dual (which needs match_gamma) is the soft form of both: the dual kernel's col_idx serves the filter and this returns False."""
    if match_dual:
        if match_gamma is None:
            raise ValueError("match_dual needs match_gamma (the dual softmax has a temperature)")
        if match_twoway:
            raise ValueError("match_dual already returns col_idx / col_sim; do not pass match_twoway with it")
        return False
    on = bool(match_twoway) or (pose_opts or {}).get("pair_filter", "none") == "cycle"
    if on and match_gamma is not None:
        raise ValueError("match_twoway (or pair_filter='cycle') and match_gamma: twoway and soft exclude each other (there is no soft "
                         "two-way kernel)")
    return on


def _pose_stage(model, res, cld_rgb_nrm, pose_fit, icp_iters, pose_opts, verify):
    """pose.estimate_poses, or with a `verify` dict pose.estimate_poses_verified, whose winner comes back as RT / valid beside
    verify_score f64[B], verify_which i32[B], verify_counts i32[B,C,6] and verify_cand_RT f32[B,C,3,4] (every candidate, in order);
    the dict's candidates, icp_iters, depth_iters and depth_opts are estimate_poses_verified's arguments, the rest its `verify`."""
    if verify is None:
        return pose.estimate_poses(res, cld_rgb_nrm, model.model_emb.xyz, pose_fit, icp_iters, pose_opts, _plane_normals(model, pose_opts))
    v = dict(verify)
    kw = {k: v.pop(k) for k in ("candidates", "icp_iters", "depth_iters", "depth_opts") if k in v}
    sel = pose.estimate_poses_verified(res, cld_rgb_nrm, model.model_emb.xyz, v, pose_opts=pose_opts,
                                       model_nrm=_plane_normals(model, pose_opts), **kw)
    out = dict(RT=sel["RT"], valid=sel["valid"], verify_score=sel["score"], verify_which=sel["which"], verify_counts=sel["counts"],
               verify_cand_RT=sel["cand_RT"])
    out.update((k, sel[k]) for k in ("pair_mask", "pair_count") if k in sel)
    if "depth_status" in sel:                                              # only with a "+depth" candidate
        out["verify_depth_status"] = sel["depth_status"]
    return out


def _verify_rows(verify, cid, idx, bs):
    """The verify dict of class cid ({cls_id: dict} or one dict for all), its per-instance depth / K / window cut down to rows idx."""
    if verify is None:
        return None
    v = dict(verify if "verts" in verify else verify[cid])
    for k, dims in (("depth", 3), ("K", 3), ("window", 2)):
        if torch.is_tensor(v.get(k)) and v[k].dim() == dims and v[k].shape[0] == bs:
            v[k] = v[k].index_select(0, idx)
    return v


def run_multi_object(model_dict, inputs, cls_ids, with_pose=True, precision="bf16x3", pose_fit="kabsch", icp_iters=0, pose_opts=None,
                     match_gamma=None, verify=None, match_twoway=False, match_dual=False):
    """model_dict: {cls_id: GeoMatch (eval, on the GPU)}; inputs: dict of batched device tensors (loader keys, plus
    `dpt_xyz` when the neighbour pyramid is not already in it); cls_ids: int tensor/list [bs].  pose_fit / icp_iters / pose_opts:
    pose.estimate_poses (the defaults are the plain Kabsch fit).  match_gamma: soft matching at that temperature (pipeline_step).
    verify (with_pose only): the dict pose.estimate_poses_verified takes (verts, faces, depth, K[, window, delta, ...], optionally
    candidates, icp_iters, depth_iters and depth_opts; a "+depth" candidate adds verify_depth_status), one for all classes or
    {cls_id: dict}; depth / K / window with a leading batch dimension are cut down to each class's rows.  The pose is then the verified selection and verify_score, verify_which, verify_counts join the outputs.
    match_twoway (or pair_filter="cycle" in pose_opts): two-way matching, as in pipeline_step; col_idx, col_sim (and pair_mask,
    pair_count) join the outputs.  match_dual (with match_gamma): dual-softmax matching, as in pipeline_step; col_idx, col_sim,
    col_lse, col_conf, dual join the soft outputs and pair_filter="cycle" is accepted.
    Returns dict(seg, rgbd, mesh, mask, best_idx, best_sim[, lse, conf, soft_xyz, score][, RT, valid[, icp_iters, icp_resid[, icp_status]]])."""
    twoway = _twoway(match_twoway, pose_opts, match_gamma, match_dual)
    cls = torch.as_tensor(cls_ids).cpu().tolist()
    bs = len(cls)
    out = {}
    order = []
    with torch.no_grad():
        for cid in sorted(set(cls)):
            sel = [i for i, c in enumerate(cls) if c == cid]
            idx = torch.tensor(sel, device=inputs["cld_rgb_nrm"].device)
            sub = {k: v.index_select(0, idx) for k, v in inputs.items() if torch.is_tensor(v) and v.shape[:1] == (bs,)}
            model = model_dict[cid]
            if getattr(model, "needs_pyramid", True) and "cld_nei_idx0" not in sub:
                sub.update(pyramid.build_pyramid(pyramid.cloud_from_inputs(sub["cld_rgb_nrm"]), sub["dpt_xyz"]))
            ep = model(sub)
            soft = None if match_gamma is None else dict(gamma=match_gamma, model_xyz=model.model_emb.xyz)
            res = matching.match_frames(ep, precision=precision, soft=soft, twoway=twoway, dual=match_dual)
            part = dict(seg=ep["seg"], rgbd=ep["rgbd"], mesh=ep["mesh"].expand(len(sel), -1, -1), mask=res["mask"],
                        best_idx=res["best_idx"], best_sim=res["best_sim"])
            if "col_idx" in res:
                part.update(col_idx=res["col_idx"], col_sim=res["col_sim"])
            if "dual" in res:
                part.update(col_lse=res["col_lse"], col_conf=res["col_conf"], dual=res["dual"])
            if soft is not None:
                part.update(lse=res["lse"], conf=res["conf"], soft_xyz=res["soft_xyz"], score=ops.match_score(res["conf"], res["mask"]))
            if with_pose:
                part.update(_pose_stage(model, res, sub["cld_rgb_nrm"], pose_fit, icp_iters, pose_opts, _verify_rows(verify, cid, idx, bs)))
            for k, v in part.items():
                out.setdefault(k, []).append(v)
            order += sel
    inv = torch.empty(bs, dtype=torch.long)
    inv[torch.tensor(order)] = torch.arange(bs)
    inv = inv.to(inputs["cld_rgb_nrm"].device)
    return {k: torch.cat(v, dim=0).index_select(0, inv) for k, v in out.items()}


def pipeline_step(model, inputs, precision="bf16x3", with_pose=False, keep_pyramid=False, pose_fit="kabsch", icp_iters=0, pose_opts=None,
                  match_gamma=None, verify=None, match_twoway=False, match_dual=False):
    """ONE pass of the hot path over a batch of crops resident on the device: neighbour pyramid (unless `inputs` already carries the
    loader's index arrays) -> GeoMatch.forward (eval) -> seg mask + descriptor packs + N x M arg-max (evaluator.py:78-93) [-> pose].
    Everything is enqueued on the current stream (and, with settings.USE_SIDE_STREAMS, on side streams forked from and joined back to
    it) with no host synchronisation, so the call captures in a hipGraph as it is.  Returns dict(seg, rgbd, mesh, mask, count,
    best_idx, best_sim[, RT, valid[, icp_iters, icp_resid[, icp_status]]]) plus the 30 pyramid arrays when keep_pyramid.  The pose stage is
    pose.estimate_poses(pose_fit, icp_iters, pose_opts): RANSAC and ICP run on the device too, with no host branching.
    match_gamma = None: the arg-max kernel, as ever.  With a temperature the soft kernel takes its place (same best_idx / best_sim)
    and the outputs gain lse, conf, soft_xyz (include/gdm.h gdm_match_soft_packed_hip) and score f32[B] = the mean of conf over the
    masked points (0 where none); pose_opts' weights / targets can then use them.
    verify = None: the pose stage as ever.  With with_pose and a verify dict (pose.estimate_poses_verified: verts, faces, depth, K[,
    window, delta, ...], optionally candidates, icp_iters, depth_iters and depth_opts) RT / valid are the candidate the observed depth
    agrees with best and the outputs gain verify_score, verify_which and verify_counts (verify_depth_status i32[B,C] with a "+depth"
    candidate, which pose.refine_poses_depth refines against the frame); still no host synchronisation.
    match_twoway = False: as ever.  With it (or with pair_filter="cycle" in pose_opts, which needs it) the two-way kernel takes the
    arg-max kernel's place behind the mask (same best_idx / best_sim; not together with match_gamma) and the outputs gain col_idx
    i32[B,M], col_sim f32[B,M] (include/gdm.h THE TWO-WAY RULE); the pose stage then adds pair_mask, pair_count when it filters.
    match_dual = False: as ever.  With it (it needs match_gamma) the dual kernel takes the soft kernel's place behind the mask (the
    same soft outputs, the two-way kernel's col_idx / col_sim) and the outputs gain col_lse f32[B,M], col_conf f32[B,M] and dual
    f32[B,N] (include/gdm.h THE DUAL RULE); pose_opts' weights="dual" and pair_filter="cycle" can then use them."""
    prec = _PREC[precision]
    twoway = _twoway(match_twoway, pose_opts, match_gamma, match_dual)          # refuses before anything is enqueued
    d = dict(inputs)
    pyr = None
    if not getattr(model, "needs_pyramid", True):
        ep = model(d, fused=True, defer_seg=True)          # the DGCNN variant builds its graphs inside the trunks: no pyramid
    else:
        if "cld_nei_idx0" not in d:
            pyr = pyramid.build_pyramid(pyramid.cloud_view(d["cld_rgb_nrm"]), d["dpt_xyz"], overlap=True)
            d.update(pyr)
        ep = model(d, defer_seg=True)
    B, _, N = ep["rgbd"].shape
    M = ep["mesh"].shape[-1]
    if twoway:
        mask, count, bi, bs, ci, cs = matching.match_tail(ep, B, N, M, prec, twoway=True)
        out = dict(seg=ep["seg"], rgbd=ep["rgbd"], mesh=ep["mesh"], mask=mask, count=count, best_idx=bi, best_sim=bs, col_idx=ci,
                   col_sim=cs)
    elif match_dual:
        t = matching.match_tail(ep, B, N, M, prec, soft=dict(gamma=match_gamma, model_xyz=model.model_emb.xyz), dual=True)
        out = dict(zip(ops.DUAL_KEYS, t[2:]), seg=ep["seg"], rgbd=ep["rgbd"], mesh=ep["mesh"], mask=t[0], count=t[1],
                   score=ops.match_score(t[5], t[0]))
    elif match_gamma is None:
        mask, count, bi, bs = matching.match_tail(ep, B, N, M, prec)
        out = dict(seg=ep["seg"], rgbd=ep["rgbd"], mesh=ep["mesh"], mask=mask, count=count, best_idx=bi, best_sim=bs)
    else:
        mask, count, bi, bs, lse, conf, sxyz = matching.match_tail(ep, B, N, M, prec, soft=dict(gamma=match_gamma,
                                                                                                  model_xyz=model.model_emb.xyz))
        out = dict(seg=ep["seg"], rgbd=ep["rgbd"], mesh=ep["mesh"], mask=mask, count=count, best_idx=bi, best_sim=bs, lse=lse,
                   conf=conf, soft_xyz=sxyz, score=ops.match_score(conf, mask))
    if with_pose:
        out.update(_pose_stage(model, out, d["cld_rgb_nrm"], pose_fit, icp_iters, pose_opts, verify))
    if keep_pyramid and pyr is not None:
        out.update((k, v) for k, v in pyr.items() if torch.is_tensor(v))
    return out


FRAME_KEYS = ("rgb_u8", "depth", "K", "bbox_xyxy", "mask")           # what a `frames` dict holds; the mask is optional


def frame_step(model, frames, S, n_points, seed=0, depth_fill=None, precision="bf16x3", with_pose=False, keep_pyramid=False,
               pose_fit="kabsch", icp_iters=0, pose_opts=None, match_gamma=None, match_twoway=False, match_dual=False):
    """From raw frames and detection boxes to the step's outputs: frames = dict(rgb_u8 u8[B,H,W,3], depth f32[B,H,W], K f32[B,3,3],
    bbox_xyxy f32[B,4][, mask u8[B,H,W]]) -> frontend.make_inputs_from_boxes(sampler="hash", build_pyramid=False, train=False) ->
    pipeline_step (which builds the pyramid a model needs).  seed: an int or a one-element int32 device tensor (ops.sample_assemble).
    Returns pipeline_step's dict plus choose, cld_rgb_nrm, n_valid, center, scale (and origin_labels with a mask).  Like
    pipeline_step, no host synchronisation: the call captures in a hipGraph as it is."""
    item = frontend.make_inputs_from_boxes(frames["rgb_u8"], frames["depth"], frames["K"], frames["bbox_xyxy"], S, n_points,
                                           mask=frames.get("mask"), train=False, depth_fill=depth_fill, sampler="hash", seed=seed,
                                           build_pyramid=False)
    out = pipeline_step(model, item, precision, with_pose, keep_pyramid, pose_fit, icp_iters, pose_opts, match_gamma,
                        match_twoway=match_twoway, match_dual=match_dual)
    out.update((k, item[k]) for k in ("choose", "cld_rgb_nrm", "n_valid", "center", "scale", "origin_labels") if k in item)
    return out


def outputs_equal(a, b):
    """Bit-for-bit comparison of two pipeline_step outputs (every tensor both hold).  Returns (all_equal, [names that differ])."""
    bad = [k for k in a if torch.is_tensor(a[k]) and k in b and not torch.equal(a[k], b[k])]
    return not bad, bad


class GraphedPipeline:
    """The whole step (pipeline_step) captured in a HIP graph and replayed from static input buffers: one host call per batch.

    TWO launch forms are captured and the better VALID one is what `__call__` replays (`self.form`):
      "single"  every kernel on one stream, in program order;
      "forked"  the same kernels with the neighbour pyramid, the mesh branch and the point branch on side streams
                (settings.USE_SIDE_STREAMS during the capture): parallel branches of the graph, ~12 % less time per step because the
                point branch's small kernels fill what the convolution launches leave of the chip.
    The forked form is only kept if its outputs are BIT-IDENTICAL to the single-stream EAGER step on the example inputs, after its
    first replays and again after a burst of back-to-back replays (`self.check` records every comparison); otherwise the pipeline
    falls back to the single-stream capture, and to nothing silently -- `self.form` and `self.check` say what runs.  `forked=False`
    captures the single-stream form only, `forked=True` requires the forked form (raises if it fails its check).

    All HIP operators of this package enqueue on torch's current stream with no host synchronisation and no allocation outside
    torch's graph-private pool, so they capture as they are; per-module caches (folded BN, packed weights, PReLU slopes) are filled
    by the eager warm-up passes before the capture.  Each form owns its scratch buffers (ops.BufferPool); the form that is not kept is
    freed after the decision (keep_both=True keeps both: `replay(form)`)."""

    def __init__(self, model, example_inputs, precision="bf16x3", with_pose=True, warmup=3, forked="auto", burst=8,
                 keep_pyramid=False, capture_error_mode=None, keep_both=False, pose_fit="kabsch", icp_iters=0, pose_opts=None,
                 match_gamma=None, match_twoway=False, match_dual=False):
        self.model = model.eval()
        self.match_gamma, self.match_twoway, self.match_dual = match_gamma, match_twoway, match_dual
        self.precision, self.with_pose, self.keep_pyramid = precision, with_pose, keep_pyramid
        self.pose_fit, self.icp_iters, self.pose_opts = pose_fit, icp_iters, dict(pose_opts or {})
        self.static_in = {k: v.clone() for k, v in example_inputs.items() if torch.is_tensor(v)}
        self.graphs, self.outs, self.pools, self.check = {}, {}, {}, {}
        self._cap_kw = {"capture_error_mode": capture_error_mode} if capture_error_mode else {}
        caller_forked = bool(settings.USE_SIDE_STREAMS)     # the caller switched the forks on globally: capture as told, one form
        with torch.no_grad():
            if caller_forked:
                self._capture("forked", warmup)
                self.form = "forked"
            else:
                ref = self._eager_reference(warmup)
                self._capture("single", 1)
                self.check["single"] = self._compare(ref, "single", burst)
                self.form = "single"
                if forked in ("auto", True):
                    try:
                        settings.USE_SIDE_STREAMS = True
                        self._capture("forked", 2)
                        self.check["forked"] = self._compare(ref, "forked", burst)
                    except Exception as e:                              # noqa: BLE001 -- the forked form is a candidate only
                        torch.cuda.synchronize()
                        self.check["forked"] = {"bit_identical": False,
                                                "error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")}
                        self.graphs.pop("forked", None)
                    finally:
                        settings.USE_SIDE_STREAMS = False
                    if self.check["forked"].get("bit_identical"):
                        self.form = "forked"
                    else:
                        self.graphs.pop("forked", None)
                        self.outs.pop("forked", None)
                        if forked is True:
                            raise RuntimeError("GraphedPipeline(forked=True): the forked capture is not bit-identical to the eager "
                                               "step: %r" % (self.check["forked"],))
        self.graph = self.graphs[self.form]
        self.static_out = self.outs[self.form]
        if not keep_both:                                            # the capture that lost keeps its private memory pool (activations of a
            for f in [f for f in self.graphs if f != self.form]:     # whole step): drop it unless the caller wants to time both (bench.py)
                del self.graphs[f], self.outs[f]
                self.pools.pop(f, None)

    # -- construction helpers ---------------------------------------------------------------------------------------------
    def _step(self):
        return pipeline_step(self.model, self.static_in, self.precision, self.with_pose, self.keep_pyramid, self.pose_fit, self.icp_iters,
                             self.pose_opts, self.match_gamma, match_twoway=self.match_twoway, match_dual=self.match_dual)

    def _eager_reference(self, warmup):
        """Eager single-stream steps on the example inputs (they also fill the per-module caches); the last one's outputs, cloned."""
        pool = self.pools.setdefault("single", ops.BufferPool())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), ops.buffer_pool(pool):
            for _ in range(max(warmup, 1)):
                out = self._step()
            ref = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        return ref

    def _capture(self, form, warmup):
        pool = self.pools.setdefault(form, ops.BufferPool())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), ops.buffer_pool(pool):
            for _ in range(warmup):                                  # the form's scratch buffers (and side-stream allocations) exist
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, **self._cap_kw), ops.buffer_pool(pool):
            out = self._step()
        self.graphs[form], self.outs[form] = g, out

    def _compare(self, ref, form, burst):
        g, out = self.graphs[form], self.outs[form]
        g.replay()
        g.replay()                                                   # twice: the second replay also reads what the first left behind
        torch.cuda.synchronize()
        ok1, bad1 = outputs_equal(ref, out)
        for _ in range(burst):                                       # back to back, no synchronisation in between
            g.replay()
        torch.cuda.synchronize()
        ok2, bad2 = outputs_equal(ref, out)
        return {"bit_identical": bool(ok1 and ok2), "first_replays_equal_eager": bool(ok1), "after_burst_equal_eager": bool(ok2),
                "burst": burst, "differing": sorted(set(bad1 + bad2))}

    # -- use --------------------------------------------------------------------------------------------------------------
    def __call__(self, inputs):
        """Copies `inputs` into the static buffers, replays the graph, returns the static outputs (valid until the next call)."""
        for k, buf in self.static_in.items():
            buf.copy_(inputs[k], non_blocking=True)
        self.graph.replay()
        return self.static_out

    def replay(self, form=None):
        """One replay of a captured form on the static inputs (default: the form __call__ uses); returns that form's static outputs."""
        form = form or self.form
        self.graphs[form].replay()
        return self.outs[form]


class GraphedFramePipeline(GraphedPipeline):
    """Frames to poses in one hipGraph replay: GraphedPipeline whose step is `frame_step`, so the front end (depth normals or depth
    completion, the box crop, the hash-sampled item) is captured in front of the model, the matching and the pose fit.  The static
    inputs are the frame buffers (rgb_u8, depth, K, bbox_xyxy[, mask]) and a one-word seed tensor the sampling kernel reads on every
    replay: `__call__(frames, seed=None)` copies both in.  The single / forked decision and its bit-identity check against the eager
    step are GraphedPipeline's.  Works for the FFB6D model and for the DGCNN variant (needs_pyramid = False)."""

    def __init__(self, model, example_frames, S, n_points, depth_fill=None, seed=0, **kw):
        self.S, self.n_points, self.depth_fill = int(S), int(n_points), depth_fill
        dev = example_frames["depth"].device
        self.seed = torch.zeros(1, dtype=torch.int32, device=dev)
        self._set_seed(seed)
        super().__init__(model, {k: example_frames[k] for k in FRAME_KEYS if example_frames.get(k) is not None}, **kw)

    def _set_seed(self, seed):
        s = int(seed) & 0xffffffff
        self.seed.fill_(s - (1 << 32) if s >= (1 << 31) else s)         # the 32-bit word, as the int32 the tensor holds

    def _step(self):
        return frame_step(self.model, self.static_in, self.S, self.n_points, self.seed, self.depth_fill, self.precision, self.with_pose,
                          self.keep_pyramid, self.pose_fit, self.icp_iters, self.pose_opts, self.match_gamma, self.match_twoway, self.match_dual)

    def __call__(self, frames, seed=None):
        """Copies `frames` (and, when given, the seed) into the static buffers, replays the graph, returns the static outputs (valid
        until the next call)."""
        if seed is not None:
            self._set_seed(seed)
        return super().__call__(frames)
