"""What FFB6DEmb computes, as hashes, for comparing two source trees (run it with each tree's root as the working directory):
  eval    the embedding of the headline model (batch 2, N = 2048; the fixture of tests/test_gpu_fused_passes.py) under the defaults and
          with each switch off that moves a fusion site to another form, point lane on the current stream (1) and on a side stream (2),
          each forward run twice: sha256 of both returned halves, and the peak memory of the one-lane default forward at batch 16;
  train   one training step of tests/test_gpu_train_replay.py's step (B = 2, N = 1024, M = 512, fixed seeds), run twice: the loss, one
          sha256 over every parameter gradient in named_parameters() order, peak memory.
--save DIR keeps the tensors (DIR/eval.pt, DIR/train.pt) so that a differing pair can be measured: --diff DIR_A DIR_B prints the largest
absolute difference per entry.  profiles/fusion_paths.md was written from this."""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
SETTINGS = [None, "USE_MFMA_GEMM", "USE_POINTWISE", "USE_PACKED_PRODUCERS", "USE_SPARSE_FINAL", "USE_FUSED_UPCONV"]


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def eval_hashes(keep):
    from geometric_aware_dense_matching_amd import pyramid, settings, synthetic
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    N, M = 2048, 8192
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join("tests", "golden", "geomatch_state.json")))
    model.load_state_dict(synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0), strict=False)
    emb = model.pcd_emb.cuda().eval()

    def inputs(B):
        batch = synthetic.make_batch(seed=100, batch=B, n_points=N)
        d = {k: torch.from_numpy(batch[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose")}
        d.update(pyramid.build_pyramid(pyramid.cloud_from_inputs(d["cld_rgb_nrm"]), torch.from_numpy(batch["dpt_xyz"]).cuda()))
        torch.cuda.synchronize()
        return d
    d = inputs(2)
    settings.SIDE_PARTS = ["point"]
    for off in SETTINGS:
        if off:
            setattr(settings, off, False)
        for lanes in (1, 2):
            settings.USE_SIDE_STREAMS = lanes == 2
            for run in (1, 2):
                with torch.no_grad():
                    a, b = [v.clone() for v in emb(dict(d), parts=True)]
                torch.cuda.synchronize()
                print("eval %-22s lanes %d run %d  image %s  point %s  finite %s" % (
                    off or "default", lanes, run, sha(a), sha(b), bool(torch.isfinite(a).all() and torch.isfinite(b).all())), flush=True)
                keep["%s/%d/%d" % (off or "default", lanes, run)] = (a.cpu(), b.cpu())
        if off:
            setattr(settings, off, True)
        print("eval %-22s allocated afterwards %d bytes" % (off or "default", torch.cuda.memory_allocated()), flush=True)
    settings.USE_SIDE_STREAMS = False
    d = inputs(16)
    for run in (1, 2):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            emb(dict(d), parts=True)
        torch.cuda.synchronize()
        print("eval batch 16, one lane, run %d: peak memory above the inputs %d bytes, allocated afterwards %d bytes" % (
            run, torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated()), flush=True)


def train_hashes(keep):
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import test_gpu_train_replay as t
    model = t._ffb6d(False)
    for run in (1, 2):
        from geometric_aware_dense_matching_amd import train_lm
        ds = train_lm.SyntheticCrops(t.B, t.N, t.M, seed=5)
        batch = torch.utils.data.default_collate([ds[i] for i in range(t.B)])
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        torch.cuda.reset_peak_memory_stats()
        out, _ = train_lm.model_fn_dec(model, batch, torch.device("cuda", 0))
        out["loss"].backward()
        torch.cuda.synchronize()
        grads = [(n, p.grad) for n, p in model.named_parameters() if p.grad is not None]
        print("train run %d  loss %s (%r)  %d gradients %s  peak memory %d bytes" % (
            run, sha(out["loss"]), float(out["loss"].detach()), len(grads), sha(*[g for _, g in grads]), torch.cuda.max_memory_allocated()), flush=True)
        keep["run%d" % run] = {"loss": out["loss"].detach().cpu(), **{n: g.cpu() for n, g in grads}}


def diff(a, b):
    """Per entry: equal or not, the largest |difference|, the largest of max|difference| / max|value| over the entry's tensors, and the relative L2 distance of all of them taken as one vector."""
    for name in ("eval.pt", "train.pt"):
        if not (os.path.exists(os.path.join(a, name)) and os.path.exists(os.path.join(b, name))):
            continue
        x, y = torch.load(os.path.join(a, name)), torch.load(os.path.join(b, name))
        for k in x:
            xs, ys = (x[k], y[k]) if isinstance(x[k], tuple) else (list(x[k].values()), list(y[k].values()))
            names = ("image", "point") if isinstance(x[k], tuple) else list(x[k])
            d = [float((p.double() - q.double()).abs().max()) for p, q in zip(xs, ys)]
            rel = [di / max(float(p.abs().max()), 1e-30) for di, p in zip(d, xs)]
            w = max(range(len(d)), key=lambda i: rel[i])
            l2 = (sum(float((p.double() - q.double()).pow(2).sum()) for p, q in zip(xs, ys)) / sum(float(p.double().pow(2).sum()) for p in xs)) ** 0.5
            print("%s %-28s %s  max |d| = %.3g  worst max|d|/max|x| = %.3g (%s)  ||d|| / ||x|| over all = %.3g  tensors that differ: %d of %d" % (
                name, k, "equal" if all(torch.equal(p, q) for p, q in zip(xs, ys)) else "DIFFER", max(d), rel[w], names[w], l2,
                sum(1 for p, q in zip(xs, ys) if not torch.equal(p, q)), len(xs)))


if __name__ == "__main__":
    if "--diff" in sys.argv:
        i = sys.argv.index("--diff")
        diff(sys.argv[i + 1], sys.argv[i + 2])
        sys.exit(0)
    save = sys.argv[sys.argv.index("--save") + 1] if "--save" in sys.argv else None
    for what, fn in (("eval", eval_hashes), ("train", train_hashes)):
        if what in sys.argv:
            keep = {}
            fn(keep)
            if save:
                os.makedirs(save, exist_ok=True)
                torch.save(keep, os.path.join(save, what + ".pt"))
