#!/usr/bin/env python3
"""train_lm.py / train_ycb.py entry-point surface of the reference, on the MI355X path.

Same single-dash flags as /root/reference/train_lm.py:35-86 (`-state {train,test,eval} -cls_id -dataset_name
-checkpoint --gpus --local_rank --gpu --deterministic -weight_decay -bn_momentum -bn_decay -decay_step`), same
checkpoint layout, same optimiser / schedulers (Adam 1e-4, CyclicLR 1e-6..1e-3 triangular, BN momentum decay),
SyncBN + DDP over RCCL.  Launch as the reference does (train_lm.sh:8), e.g.
    python -m torch.distributed.run --nproc_per_node=8 -m geometric_aware_dense_matching_amd.train_lm \\
        --gpus=8 -state=train -dataset_name=lmo -cls_id=1 -checkpoint=train_log/lm/checkpoints/

`-dataset_name {lmo,ycbv}` selects the configuration the reference imports at module top (config/<name>_cfg.py:
diameters, neighbour radius factor, key-point and checkpoint directories, object list, batch sizes, strict / non-strict
checkpoint loading); `--model-variant dgcnn` builds models/geoMatch_DGCNN.py's GeoMatch instead of the FFB6D + SplineCNN one.

Three things differ by design:
  * the neighbour pyramid is built on the GPU inside `model_fn_dec` (two launches per batch) instead of 22
    KD-tree calls per crop in the DataLoader workers;
  * `test()` keeps one model per object of the dataset like the reference (train_lm.py:331-340) but runs the instances of a
    batch GROUPED per object (infer.run_multi_object) instead of one batch-1 forward per instance (:298-314), with the
    input-independent mesh descriptors cached per object;
  * BOP dataset loaders are out of scope: `-data synthetic` (default) feeds generated crops
    with the loader's item layout, `-data rendered` feeds RGB-D frames of the object's mesh drawn on the GPU (render.py), a real
    loader can be plugged through `--dataset-factory module:function`.
"""
import argparse
import importlib
import os
import time

import numpy as np
import torch
import torch.nn as nn

from . import infer, matching, ops, pose, pyramid, settings, synthetic
from .checkpoint import load_checkpoint, save_checkpoint
from .config import LMO_OBJS as LM_OBJS, dataset_config, make_dgcnn_cfg, make_model_cfg
from .geoMatch import GeoMatch
from .parallel import init_distributed, wrap_for_training

bnm_clip = 1e-2
DEFAULT_DATASET = "lmo"                     # train_ycb.py sets "ycbv" (train_ycb.py:70)


GT_TARGETS = ("loader", "device")


def build_parser():
    p = argparse.ArgumentParser(description="Arg parser")
    p.add_argument("-weight_decay", type=float, default=0)
    p.add_argument("-lr", type=float, default=1e-2)
    p.add_argument("-lr_decay", type=float, default=0.5)
    p.add_argument("-decay_step", type=float, default=2e5)
    p.add_argument("-bn_momentum", type=float, default=0.9)
    p.add_argument("-bn_decay", type=float, default=0.5)
    p.add_argument("-checkpoint", type=str, default=None)
    p.add_argument("-state", type=str, default="eval")
    p.add_argument("-dataset_name", type=str, default=DEFAULT_DATASET)
    p.add_argument("-cls_id", type=int, default=5)
    p.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    p.add_argument("-n", "--nodes", default=1, type=int)
    p.add_argument("-g", "--gpus", default=8, type=int)
    p.add_argument("-nr", "--nr", default=0, type=int)
    p.add_argument("--gpu", type=str, default=None)
    p.add_argument("--deterministic", action="store_true")
    # additions (not in the reference)
    p.add_argument("-data", type=str, default="synthetic", choices=["synthetic", "rendered"],
                   help="synthetic = generated crops (random surfaces, nothing to learn); rendered = RGB-D frames of the object's mesh "
                        "drawn on the GPU (render.RenderedFrames) -- the meshes of --models-dir, or render.demo_mesh without it; implies "
                        "--gt-targets device and, with -state=test, --single-object on held-out frames (another seed)")
    p.add_argument("--dataset-factory", type=str, default=None, help="module:function(cfg, split) -> torch Dataset")
    p.add_argument("--model-variant", type=str, default="ffb6d", choices=["ffb6d", "dgcnn"],
                   help="ffb6d = models/geoMatch.py (CNN + RandLA + SplineCNN); dgcnn = models/geoMatch_DGCNN.py")
    p.add_argument("--epochs", type=int, default=50)
    p.add_argument("--batch-size", type=int, default=None, help="default: the dataset's TRAIN_BATCH_SIZE / VAL_BATCH_SIZE")
    p.add_argument("--n-points", type=int, default=4096)
    p.add_argument("--n-mesh", type=int, default=4096)
    p.add_argument("--synthetic-items", type=int, default=256)
    p.add_argument("--log-dir", type=str, default=None, help="default: the dataset's checkpoint directory")
    p.add_argument("--save-every", type=int, default=10)
    p.add_argument("--log-every", type=int, default=100)
    p.add_argument("--max-iters", type=int, default=None)
    p.add_argument("--single-object", action="store_true", help="test: only -cls_id instead of every object of the dataset")
    p.add_argument("--eval-output", dest="eval_output", type=str, default=None,
                   help="test: directory for the evaluator's files -- BOP result csv, error / recall / precision pickles, table text")
    p.add_argument("--bop-scores", dest="bop_scores", action="store_true",
                   help="test: also score MSSD / MSPD (BOP-2019 thresholds, AR lines) per object; written beside the recall table")
    p.add_argument("--models-info", dest="models_info", type=str, default=None,
                   help="test, with --bop-scores: the dataset's models_info.json (object symmetries); without it only the identity")
    p.add_argument("--graph-batch1", action="store_true",
                   help="test: per-object hipGraph replay for single-instance groups (a batch-1 eager step is launch-bound)")
    p.add_argument("--pose-fit", dest="pose_fit", type=str, default="kabsch", choices=["kabsch", "ransac", "consensus"],
                   help="test: pose fit from the correspondences -- least squares over all of them (evaluator.py:97), the reference's "
                        "RANSAC (pvn3d_eval_utils_kpls.py:79-124) or the consensus fit from pairwise-compatible pairs "
                        "(pose.consensus_poses), all on the GPU")
    p.add_argument("--ransac-iters", dest="ransac_iters", type=int, default=20, help="test: RANSAC hypotheses per crop (max_iter)")
    p.add_argument("--ransac-inlier-dist", dest="ransac_inlier_dist", type=float, default=0.015,
                   help="test: RANSAC inlier distance in metres (match_err)")
    p.add_argument("--consensus-tau", dest="consensus_tau", type=float, default=0.005, metavar="T",
                   help="test, --pose-fit consensus: two pairs are compatible when their scene and model distances agree within T metres "
                        "(the default of a definition, not a tuned value)")
    p.add_argument("--consensus-seeds", dest="consensus_seeds", type=int, default=8, metavar="S",
                   help="test, --pose-fit consensus: hypotheses per crop")
    p.add_argument("--consensus-inlier-dist", dest="consensus_inlier_dist", type=float, default=0.015, metavar="D",
                   help="test, --pose-fit consensus: inlier distance in metres of the hypothesis count and the refit")
    p.add_argument("--match-gamma", dest="match_gamma", type=float, default=None,
                   help="test: soft matching at this temperature (0 < G <= 40): per-point confidences, soft vertices and a csv score")
    p.add_argument("--match-dual", dest="match_dual", action="store_true",
                   help="test, with --match-gamma: dual-softmax matching (include/gdm.h THE DUAL RULE): the soft outputs, each vertex's "
                        "best masked point and the dual confidence from one pass; --pair-filter cycle then goes with --match-gamma")
    p.add_argument("--match-score", dest="match_score", type=str, default="conf", choices=["conf", "dual"],
                   help="test, --match-gamma: what the csv score averages over the masked points (dual needs --match-dual)")
    p.add_argument("--pose-weights", dest="pose_weights", type=str, default="none", choices=["none", "conf", "dual"],
                   help="test, --pose-fit kabsch: weigh the pairs by the matching confidence (needs --match-gamma) or by the dual-softmax "
                        "confidence (needs --match-dual)")
    p.add_argument("--pose-targets", dest="pose_targets", type=str, default="vertex", choices=["vertex", "soft"],
                   help="test, --pose-fit kabsch: fit to the arg-max vertex or to the expected model coordinate (needs --match-gamma)")
    p.add_argument("--pair-filter", dest="pair_filter", type=str, default="none", choices=["none", "cycle"],
                   help="test: cycle = two-way matching and the cycle-consistency pair filter in front of the fit (pose.cycle_filter); the "
                        "kept fraction of the masked points is printed per object under the recall table")
    p.add_argument("--cycle-radius", dest="cycle_radius", type=float, default=None, metavar="R",
                   help="test, --pair-filter cycle: the filter's radius in metres (default pose.CYCLE_RADIUS; 0 = mutual best pairs only)")
    p.add_argument("--icp-iters", dest="icp_iters", type=int, default=0,
                   help="test: point-to-point ICP iterations after the fit (pvn3d_eval_utils_kpls.py:126-212); 0 = none")
    p.add_argument("--icp-tolerance", dest="icp_tolerance", type=float, default=0.001,
                   help="test: ICP convergence tolerance (m); --icp-metric plane settles below a millimetre, give it 0.0001")
    p.add_argument("--icp-metric", dest="icp_metric", type=str, default="point", choices=["point", "plane"],
                   help="test: the ICP residual -- the reference's point-to-point, or point-to-plane against the model normals "
                        "(Gauss-Newton; degenerate crops are frozen and flagged in icp_status)")
    p.add_argument("--icp-huber", dest="icp_huber", type=float, default=None, metavar="M",
                   help="test, --icp-metric plane: Huber threshold on the point-to-plane residual in metres")
    p.add_argument("--icp-normal-gate", dest="icp_normal_gate", type=float, default=None, metavar="C",
                   help="test, --icp-metric plane: drop pairs whose scene and model normals have a cosine below C")
    p.add_argument("--pose-verify", dest="pose_verify", action="store_true",
                   help="test, -data rendered: fit every pose of --verify-candidates, verify each against the depth frame "
                        "(pose.estimate_poses_verified) and keep the best; prints the recall table of every candidate and of the "
                        "selection, and the verification score becomes the csv score")
    p.add_argument("--verify-delta", dest="verify_delta", type=float, default=0.01, metavar="D",
                   help="test, --pose-verify: the depth agreement tolerance in metres")
    p.add_argument("--verify-candidates", dest="verify_candidates", type=str, default="kabsch,ransac,kabsch+icp,ransac+icp",
                   help="test, --pose-verify: comma-separated candidates out of kabsch, ransac, consensus, kabsch+icp, ransac+icp, "
                        "consensus+icp "
                        "(+icp runs --icp-iters iterations, 10 when that is 0), each optionally followed by +depth: the candidate "
                        "refined against the depth frame by render-and-compare (pose.refine_poses_depth), e.g. kabsch+depth")
    p.add_argument("--depth-refine-iters", dest="depth_refine_iters", type=int, default=5, metavar="K",
                   help="test, --pose-verify: Gauss-Newton iterations of a +depth candidate")
    p.add_argument("--depth-refine-reject", dest="depth_refine_reject", type=float, default=0.01, metavar="M",
                   help="test, --pose-verify: a +depth candidate pairs a pixel whose observed depth lies within M metres of the rendered one")
    p.add_argument("--render-depth-sensor", dest="render_depth_sensor", action="store_true",
                   help="-data rendered, train and test: pass every rendered depth frame through the structured-light sensor model "
                        "(sensor.DepthSensor: range, projector shadow, grazing drop-outs, jitter, disparity noise and quantisation) "
                        "before the crop; off by default.  The --sensor-* options override its defaults")
    for _name, _help in (("baseline", "signed projector offset in metres"), ("z-min", "nearest measured depth in metres"),
                         ("z-max", "farthest measured depth in metres"), ("sigma-d", "disparity noise in pixels"),
                         ("subpixel", "disparity steps per pixel"), ("cos-min", "incidence cosine below which a pixel always drops"),
                         ("cos-soft", "incidence cosine above which a pixel never drops"),
                         ("p-shift", "probability per axis that a pixel reads its neighbour")):
        p.add_argument("--sensor-" + _name, dest="sensor_" + _name.replace("-", "_"), type=float, default=None, metavar="X",
                       help="--render-depth-sensor: " + _help)
    p.add_argument("--sensor-stages", dest="sensor_stages", type=str, default="all",
                   help="--render-depth-sensor: 'all' or a comma-separated subset of range, shadow, grazing, jitter, noise")
    p.add_argument("--objects-across-gpus", action="store_true",
                   help="train: the dataset's objects are independent jobs (train_ycb.sh:3-9 runs them one after the other): rank r of a "
                        "torch.distributed.run launch trains objects r, r + world, ... on its own GPU as single-process jobs -- no process "
                        "group, no collective")
    p.add_argument("--graph-train", action="store_true",
                   help="train: capture one iteration (forward + losses + backward + Adam) as a hipGraph and replay it (single process)")
    p.add_argument("--dgcnn-train-path", dest="dgcnn_train_path", type=str, default="modules", choices=["modules", "fused"],
                   help="train, --model-variant dgcnn: 'modules' = dense distances and library convolutions on edge tensors; 'fused' = "
                        "feature-space kNN with no N x N matrix and ops.edge_block_train stages with no edge tensor (same parameters, "
                        "interchangeable checkpoints)")
    p.add_argument("--mesh-train-path", dest="mesh_train_path", type=str, default="dense", choices=["dense", "grouped"],
                   help="train: how the SplineConv layers of the mesh branch run (splinecnn.SplineCNN_Mesh.train_path): 'dense' = the "
                        "[M, 125*C] table on the library GEMM with an atomic backward; 'grouped' = the edge-grouped launches of inference "
                        "with a gather-form backward, no table, reproducible gradients (same parameters, interchangeable checkpoints)")
    p.add_argument("--gt-targets", dest="gt_targets", type=str, default="loader", choices=GT_TARGETS,
                   help="train: 'loader' = labels / match_idx / visible_flag come with the items; 'device' = computed on the GPU from the "
                        "items' RT and origin_labels (get_pose_gt_info, linemod_pbr.py:602-655; targets.pose_gt_info), invalid items "
                        "replaced by the batch's first valid one")
    p.add_argument("--soft-gamma", dest="soft_gamma", type=float, default=16.0,
                   help="train: temperature of the soft-assignment losses (0 < gamma <= 40; loss.SoftAssignLoss)")
    p.add_argument("--soft-xyz-weight", dest="soft_xyz_weight", type=float, default=0.0,
                   help="train: weight of the expected-vertex regression (smooth L1, metres) added to the loss; 0 = off")
    p.add_argument("--soft-nll-weight", dest="soft_nll_weight", type=float, default=0.0,
                   help="train: weight of the negative log-likelihood of the ground-truth vertex under the soft assignment; 0 = off")
    p.add_argument("--pose-loss-weight", dest="pose_loss_weight", type=float, default=0.0,
                   help="train: weight of the pose-fit loss (loss.PoseFitLoss: the ADD-style error of the weighted Kabsch fit of the soft "
                        "vertices at --soft-gamma against the item's RT, differentiable through own kernels); 0 = off")
    p.add_argument("--pose-loss-points", dest="pose_loss_points", type=int, default=256, metavar="K",
                   help="train: the pose-fit loss measures the first K model points (a farthest-point subset by the model file's contract)")
    p.add_argument("--pose-loss-weights", dest="pose_loss_weights", type=str, default="uniform", choices=["uniform", "prob"],
                   help="train: fit weights of the pose-fit loss: 'uniform' = the selected rows, 'prob' = the soft assignment's probability "
                        "of the ground-truth vertex")
    p.add_argument("--models-dir", dest="models_dir", type=str, default=None, metavar="DIR",
                   help="a BOP models directory: when the dataset has no obj_%%06d_fps.npy for an object and DIR/obj_%%06d.ply exists, "
                        "the model table is built from that mesh on the GPU (model_prep.build_model_points) instead of a synthetic one")
    return p


def _set_soft_losses(model, args):
    """--soft-gamma / --soft-xyz-weight / --soft-nll-weight onto the model; with both weights 0 the class defaults stay untouched."""
    wx, wn = float(getattr(args, "soft_xyz_weight", 0.0)), float(getattr(args, "soft_nll_weight", 0.0))
    if wx != 0 or wn != 0:
        model.soft_gamma, model.soft_xyz_weight, model.soft_nll_weight = float(getattr(args, "soft_gamma", 16.0)), wx, wn
    wp = float(getattr(args, "pose_loss_weight", 0.0))
    if wp != 0:          # --pose-loss-weight / --pose-loss-points / --pose-loss-weights; its targets are the soft vertices at --soft-gamma
        model.soft_gamma, model.pose_loss_weight = float(getattr(args, "soft_gamma", 16.0)), wp
        model.pose_loss_points, model.pose_loss_weights = int(getattr(args, "pose_loss_points", 256)), getattr(args, "pose_loss_weights", "uniform")
    return model


class BNMomentumScheduler:
    """models/pytorch_utils.py:486-505.  As in the reference the setter matches BatchNorm1d/2d/3d only (:478-481): the reference
    converts to SyncBatchNorm BEFORE it builds the scheduler (train_lm.py:412,449-457), so under DDP the SyncBN layers keep their
    constructor momentum (0.1; 0.99 for RandLA's layers) and only single-process runs see the decay."""

    def __init__(self, model, bn_lambda, last_epoch=-1):
        self.model, self.lmbd = model, bn_lambda
        self.step(last_epoch + 1)
        self.last_epoch = last_epoch

    def step(self, epoch=None):
        if epoch is None:
            epoch = self.last_epoch + 1
        self.last_epoch = epoch
        m = self.lmbd(epoch)
        for mod in self.model.modules():
            if type(mod) in (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d):
                mod.momentum = m


class SyntheticCrops(torch.utils.data.Dataset):
    """Generated items with the loader's keys (datasets/lm/linemod_pbr.py:572-599): model inputs + labels,
    match_idx (index of the corresponding model vertex, M = 'no correspondence'), visible_flag, RT."""

    def __init__(self, n_items, n_points, n_mesh, seed=0, cls_ids=None, with_ids=True, *, model_xyz=None):
        self.n_items, self.n_points, self.n_mesh, self.seed = n_items, n_points, n_mesh, seed
        self.cls_ids = list(cls_ids) if cls_ids else None          # test split: item i is an instance of cls_ids[i % len]
        self.with_ids = with_ids                                    # scene_id / im_id as a BOP test split carries them (evaluator.py:366-367)
        # --gt-targets device: the object model f32[M,3] (m); items then carry a ground-truth pose and points on the posed model
        self.model_xyz = None if model_xyz is None else np.asarray(model_xyz, dtype=np.float32)

    def __len__(self):
        return self.n_items

    def __getitem__(self, i):
        if self.model_xyz is not None:
            return self._posed_item(i)
        it = synthetic.make_crop(self.seed * 100003 + i, self.n_points)
        rs = np.random.RandomState(self.seed * 7 + i)
        labels = it["labels"].astype(np.int32)
        match = rs.randint(0, self.n_mesh, size=self.n_points).astype(np.int32)
        match[rs.rand(self.n_points) < 0.1] = self.n_mesh
        it.update(labels=labels, origin_labels=labels.copy(), match_idx=match, visible_flag=(rs.rand(self.n_mesh) < 0.6).astype(np.uint8),
                  RT=np.eye(4, dtype=np.float32)[:3])
        if self.cls_ids:
            it["cls_id"] = np.int32(self.cls_ids[i % len(self.cls_ids)])
        if self.with_ids:
            it["scene_id"], it["im_id"] = np.int32(1 + self.seed), np.int32(i)
        return it

    def _posed_item(self, i):
        """An item for --gt-targets device: a pose RT (model -> camera, 0.5-1.2 m away) and labelled points on the posed model --
        camera-facing vertices plus 1-2 mm noise, about 10 % pushed 1.5-3 cm outwards -- written over the crop's labelled points.
        Ships RT and origin_labels; labels / match_idx / visible_flag are computed on the device."""
        it = synthetic.make_crop(self.seed * 100003 + i, self.n_points)
        rs = np.random.RandomState(self.seed * 7 + i + 7919)
        q, _ = np.linalg.qr(rs.randn(3, 3))
        q *= np.sign(np.linalg.det(q))
        t = np.array([rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1), rs.uniform(0.5, 1.2)])
        RT = np.concatenate([q, t[:, None]], axis=1).astype(np.float32)
        posed = self.model_xyz @ RT[:, :3].T + RT[:, 3]
        front = np.where(posed[:, 2] < np.median(posed[:, 2]))[0]
        lab = np.where(it["labels"] > 0)[0]
        pick = rs.choice(front, size=len(lab))
        d = rs.randn(len(lab), 3)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        off = rs.uniform(0.001, 0.002, size=(len(lab), 1))
        far = rs.rand(len(lab)) < 0.1
        out = posed[pick[far]] - posed.mean(0)
        d[far] = out / np.linalg.norm(out, axis=1, keepdims=True)
        off[far, 0] = rs.uniform(0.015, 0.03, size=int(far.sum()))
        it["cld_rgb_nrm"][:3, lab] = (posed[pick] + d * off).T.astype(np.float32)
        labels = it.pop("labels").astype(np.int32)
        it.update(origin_labels=labels, RT=RT)
        if self.cls_ids:
            it["cls_id"] = np.int32(self.cls_ids[i % len(self.cls_ids)])
        if self.with_ids:
            it["scene_id"], it["im_id"] = np.int32(1 + self.seed), np.int32(i)
        return it


def to_device(data, device):
    """model_fn_dec's dtype rules (train_lm.py:158-172); int tensors stay int32 (the HIP ops take them as is)."""
    out = {}
    for k, v in data.items():
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(v)
        if not torch.is_tensor(v):
            out[k] = v
            continue
        if v.dtype in (torch.float32, torch.uint8, torch.float64):
            out[k] = v.float().to(device, non_blocking=True)
        elif v.dtype in (torch.int32, torch.int16, torch.int64):
            out[k] = v.to(torch.int32).to(device, non_blocking=True)
        else:
            out[k] = v.to(device)
    return out


def device_targets(model, cu, counter=None):
    """--gt-targets device: labels / match_idx / visible_flag of every item from its RT and origin_labels and the model's own
    vertices (targets.pose_gt_info, get_pose_gt_info of linemod_pbr.py:602-655), in the loader's dtypes.  The reference draws another
    item for an invalid one (:509-510, :663-668); a batch has a fixed shape here, so every invalid item is replaced by the batch's
    first valid item (a device gather over every batch tensor), and a batch without any valid item is left as it is.  counter i64[2]
    (device, optional) += (items replaced, items of batches without a valid item).  No host synchronisation."""
    from . import targets
    emb = getattr(model, "module", model).model_emb
    B = cu["RT"].shape[0]
    gt = targets.pose_gt_info(cu["cld_rgb_nrm"], cu["origin_labels"], cu["RT"], emb.xyz.contiguous())
    cu["labels"] = gt["labels"].to(torch.int32)
    cu["match_idx"] = gt["match_idx"]
    cu["visible_flag"] = gt["visible_flag"].float()
    valid = gt["valid"]
    ar = torch.arange(B, device=valid.device)
    any_valid = valid.any()
    first = torch.argmax(valid.to(torch.float32))                    # lowest index of a valid item (0 when there is none)
    src = torch.where(valid | ~any_valid, ar, first)
    for k, v in list(cu.items()):
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B:
            cu[k] = v.index_select(0, src)
    if counter is not None:
        n_bad = (~valid).sum()
        counter += torch.stack([torch.where(any_valid, n_bad, 0), torch.where(any_valid, 0, n_bad)]).to(counter.dtype)
    return cu


def model_fn_dec(model, data, device, gt_targets="loader", counter=None):
    cu = to_device(data, device)
    if gt_targets == "device":
        cu = device_targets(model, cu, counter)
    elif gt_targets != "loader":
        raise ValueError("gt_targets must be one of %s, got %r" % (GT_TARGETS, gt_targets))
    needs_pyramid = getattr(getattr(model, "module", model), "needs_pyramid", True)       # the DGCNN variant builds its own graphs
    if needs_pyramid and "cld_nei_idx0" not in cu:            # pyramid on the GPU (two launches per batch)
        cu.update(pyramid.build_pyramid(pyramid.cloud_from_inputs(cu["cld_rgb_nrm"]), cu["dpt_xyz"]))
    with ops.batched_bn_counters():                       # the 91 BatchNorm step counters as one multi-tensor add
        return model(cu), cu


class Trainer:
    """train_lm.py:178-296."""

    def __init__(self, model, optimizer, checkpoint_dir, obj_name, lr_scheduler=None, bnm_scheduler=None, device=None,
                 local_rank=0, save_every=10, log_every=100, graphed_step=None, gt_targets="loader"):
        self.model, self.optimizer = model, optimizer
        self.gt_targets = gt_targets
        # --gt-targets device: (items replaced, items of batches without a valid item), on the device, read with the loss sums
        self.replaced = torch.zeros(2, dtype=torch.int64, device=device) if gt_targets == "device" else None
        self.graphed_step = graphed_step                     # train_graph.GraphedTrainStep: the iteration as one hipGraph launch
        self.lr_scheduler, self.bnm_scheduler = lr_scheduler, bnm_scheduler
        self.checkpoint_dir, self.obj_name = checkpoint_dir, obj_name
        self.device, self.local_rank, self.save_every, self.log_every = device, local_rank, save_every, log_every
        self.history = []

    def train(self, start_epoch, n_epochs, train_loader, train_sampler=None, max_iters=None):
        """train_lm.py:224-296.  The reference reads three `.item()`s per iteration (:271-273), i.e. three device syncs; here the
        running sums stay on the device and are read once per `log_every` iterations (and once at the end for `history`)."""
        it_total = 0
        dev_hist = []
        try:
            for epoch in range(start_epoch, n_epochs):
                if train_sampler is not None:
                    train_sampler.set_epoch(epoch)
                sums = None
                t0 = time.time()
                for it, batch in enumerate(train_loader):
                    self.model.train()
                    if self.graphed_step is not None:
                        out = self.graphed_step.step(batch)      # forward, backward and optimizer.step() in one launch
                    else:
                        out, _ = model_fn_dec(self.model, batch, self.device, self.gt_targets, self.replaced)
                    loss = out["loss"]
                    vals = torch.stack([loss.detach().float(), out["seg_loss"].detach().float(),
                                        torch.as_tensor(out["match_loss"], device=loss.device).detach().float()]
                                       + [out[k].detach().float() for k in ("soft_xyz_loss", "soft_nll_loss", "pose_loss") if k in out])
                    sums = vals if sums is None else sums + vals
                    dev_hist.append(vals)
                    if (it + 1) % self.log_every == 0:
                        self._flush_history(dev_hist)            # the one host read of this log window; frees the per-iteration scalars
                        soft = " soft_xyz: {:.6f} soft_nll: {:.4f}" if "soft_xyz_loss" in out else ""     # the soft-assignment losses, when on
                        soft += " pose: {:.6f}" if "pose_loss" in out else ""                           # the pose-fit loss (metres), when on
                        if self.local_rank == 0 and self.replaced is not None:
                            rd = self._replaced_counter()
                            vals = torch.cat([sums / self.log_every, rd.to(sums.dtype)]).tolist()     # one read: sums and counter
                            print(("avg_loss:{:.4f} seg: {:.4f} match: {:.4f}" + soft + "  invalid items replaced: {:.0f} unreplaced: {:.0f}  "
                                   "time cost:{:.1f} s").format(*vals, time.time() - t0))
                        elif self.local_rank == 0:
                            print(("avg_loss:{:.4f} seg: {:.4f} match: {:.4f}" + soft + "  time cost:{:.1f} s").format(
                                *(sums / self.log_every).tolist(), time.time() - t0))
                        sums = None
                        t0 = time.time()
                    if self.graphed_step is None:
                        loss.backward()
                        self.optimizer.step()
                        self.optimizer.zero_grad()
                    if self.lr_scheduler is not None:
                        self.lr_scheduler.step()
                    if self.bnm_scheduler is not None:
                        self.bnm_scheduler.step()
                    it_total += 1
                    if max_iters is not None and it_total >= max_iters:
                        return it_total
                if (epoch + 1) % self.save_every == 0 and self.local_rank == 0:
                    save_checkpoint(self.model, self.optimizer, epoch, self.checkpoint_dir, self.obj_name)
            return it_total
        finally:
            self._flush_history(dev_hist)

    def _replaced_counter(self):
        """The device counter of invalid items (eager loop's, or the graphed step's own)."""
        if self.graphed_step is not None and self.graphed_step.replaced is not None:
            return self.graphed_step.replaced
        return self.replaced

    HISTORY_CAP = 100000          # `history` keeps the most recent iterations' (loss, seg, match[, soft_xyz, soft_nll][, pose]) tuples

    def _flush_history(self, dev_hist):
        if dev_hist:
            self.history += [tuple(v) for v in torch.stack(dev_hist).cpu().tolist()]
            dev_hist.clear()
            if len(self.history) > self.HISTORY_CAP:
                del self.history[:len(self.history) - self.HISTORY_CAP]


RENDERED_DISTRACTORS = 3          # -data rendered --models-dir: at most this many other meshes of DIR are drawn beside the object


def _rendered_meshes(args, cls_id):
    """-data rendered: ([mesh dicts in the model file's unit (mm)], index of object cls_id).  With --models-dir the object's
    obj_%06d.ply and up to RENDERED_DISTRACTORS other meshes of DIR; without it render.demo_mesh(seed=cls_id) and a second demo mesh."""
    from . import model_prep, render
    models_dir = getattr(args, "models_dir", None)
    if not models_dir:
        out = []
        for seed in (cls_id, cls_id + 1000):
            m = render.demo_mesh(level=3, seed=seed)
            out.append(dict(m, verts=m["verts"] * 1000.0))
        return out, 0
    ply = os.path.join(models_dir, "obj_%06d.ply" % cls_id)
    if not os.path.exists(ply):
        raise SystemExit("-data rendered: %s does not exist" % ply)
    others = sorted(f for f in os.listdir(models_dir) if f.startswith("obj_") and f.endswith(".ply") and f != os.path.basename(ply))
    out = []
    for path in [ply] + [os.path.join(models_dir, f) for f in others[:RENDERED_DISTRACTORS]]:
        out.append(model_prep.load_mesh(path, verbose=True))               # with its texture, when the file names one beside it
    return out, 0


def depth_sensor_from_args(args):
    """--render-depth-sensor and the --sensor-* overrides -> a sensor.DepthSensor, or None with the option off."""
    if not getattr(args, "render_depth_sensor", False):
        return None
    from . import sensor
    over = {k: getattr(args, "sensor_" + k, None) for k in ("baseline", "z_min", "z_max", "sigma_d", "subpixel", "cos_min", "cos_soft",
                                                            "p_shift")}
    stages = getattr(args, "sensor_stages", "all") or "all"
    return sensor.DepthSensor(stages="all" if stages == "all" else [s.strip() for s in stages.split(",") if s.strip()],
                              **{k: v for k, v in over.items() if v is not None})


def make_rendered(args, split, cls_id, batch_size, device, keep_frames=False):
    """-data rendered: render.RenderedFrames over the object's mesh (metres), other meshes as distractors and a backdrop plane;
    --synthetic-items frames per epoch; the test split draws from another seed and carries no box jitter.  keep_frames: the batches
    also carry the depth frame and the target's box (--pose-verify).  --render-depth-sensor: both splits see sensed depth."""
    from . import render
    meshes, target = _rendered_meshes(args, cls_id)
    packed = [render._as_mesh(m) for m in meshes]
    packed.append(render._as_mesh(render.backdrop_mesh(synthetic.LM_K, 480, 640, z=1500.0)))
    scene = render.SceneMeshes(packed, device=device, scale=0.001)
    ds = dataset_config(args.dataset_name)
    model_xyz = _model_points(args, ds, cls_id)[:, :3] / 1000.0
    return render.RenderedFrames(scene, target, model_xyz, batch_size, args.n_points, seed=0 if split == "train" else 1,
                                 n_batches=max(1, args.synthetic_items // batch_size), backdrop_obj=len(packed) - 1,
                                 train=split == "train", cls_id=cls_id, keep_frames=keep_frames,
                                 depth_sensor=depth_sensor_from_args(args))


def make_dataset(args, split, cls_ids=None):
    if args.dataset_factory:
        mod, fn = args.dataset_factory.split(":")
        return getattr(importlib.import_module(mod), fn)(args, split)
    model_xyz = None
    if split == "train" and getattr(args, "gt_targets", "loader") == "device":
        ds = dataset_config(args.dataset_name)
        model_xyz = _model_points(args, ds, args.cls_id)[:, :3] / 1000.0           # the model_emb.xyz of build_model (metres)
    return SyntheticCrops(args.synthetic_items, args.n_points, args.n_mesh, seed=0 if split == "train" else 1, cls_ids=cls_ids,
                          model_xyz=model_xyz)


def _model_points(args, ds, cls_id):
    if getattr(args, "data", "synthetic") == "rendered":                    # the table of the mesh that is drawn, never another one
        from . import model_prep
        return model_prep.build_model_points(_rendered_meshes(args, cls_id)[0][0], args.n_mesh)
    path = os.path.join(ds["model_pth"], "obj_%06d_fps.npy" % cls_id)
    if os.path.exists(path):
        return np.load(path)
    ply = os.path.join(getattr(args, "models_dir", None) or "", "obj_%06d.ply" % cls_id)
    if getattr(args, "models_dir", None) and os.path.exists(ply):          # --models-dir: the table built from the BOP mesh, in memory
        from . import model_prep
        return model_prep.build_model_points(ply, args.n_mesh)
    return synthetic.make_model_points(cls_id, args.n_mesh, ds["diameters"][cls_id])       # KeyError: not an object of this dataset


def build_model(args, cls_id, cache_mesh_in_eval=False):
    """GeoMatch(cfg.MODEL, cls_id) of the selected dataset and variant (train_lm.py:410, :332)."""
    ds = dataset_config(args.dataset_name)
    if cls_id not in ds["diameters"]:
        raise KeyError("-cls_id=%d is not an object of -dataset_name=%s (ids %s)" % (cls_id, args.dataset_name, sorted(ds["diameters"])))
    pts = _model_points(args, ds, cls_id)
    if args.model_variant == "dgcnn":
        from .geoMatch_DGCNN import GeoMatch as GeoMatchDGCNN
        model = GeoMatchDGCNN(make_dgcnn_cfg(n_mesh_node=args.n_mesh, dataset=args.dataset_name), cls_id, model_points=pts)
        model.train_path = getattr(args, "dgcnn_train_path", "modules")
        return _set_soft_losses(_set_mesh_train_path(model, args), args)
    cfg = make_model_cfg(n_mesh_node=args.n_mesh, num_points=args.n_points, dataset=args.dataset_name)
    return _set_soft_losses(_set_mesh_train_path(GeoMatch(cfg, cls_id, model_points=pts, cache_mesh_in_eval=cache_mesh_in_eval), args), args)


def _set_mesh_train_path(model, args):
    """--mesh-train-path onto the model's SplineCNN mesh branch, where the variant has one."""
    from .splinecnn import SplineCNN_Mesh
    emb = getattr(model, "model_emb", None)
    if isinstance(emb, SplineCNN_Mesh):
        emb.train_path = getattr(args, "mesh_train_path", "dense")
    return model


def obj_name_of(ds, cls_id):
    return ds["objs"].get(cls_id, "obj_%02d" % cls_id)


def object_shard(cls_ids, rank, world):
    """Objects of rank `rank` under --objects-across-gpus: every world-th object of the sorted id list (disjoint, covering)."""
    return sorted(cls_ids)[rank::world]


def train_objects_across_gpus(args):
    """The zero-communication sharding of BASELINE config 3: the 21 YCB-V (8 LM-O) objects are independent training jobs
    (/root/reference/train_ycb.sh:3-9), so each rank of the launch trains its share of them alone on its GPU.  Returns
    {cls_id: Trainer}."""
    import copy
    from .parallel import env_rank
    rank, local_rank, world = env_rank()
    ds = dataset_config(args.dataset_name)
    mine = object_shard(ds["objs"], rank, world)
    out = {}
    for cid in mine:
        a = copy.copy(args)
        a.cls_id, a.local_rank, a.objects_across_gpus, a._single_process = cid, local_rank, False, True
        print("[rank %d/%d] training object %d (%s)" % (rank, world, cid, obj_name_of(ds, cid)), flush=True)
        out[cid] = train(a)
    return out


def train(args):
    if getattr(args, "objects_across_gpus", False):
        return train_objects_across_gpus(args)
    torch.backends.cudnn.benchmark = not args.deterministic
    if args.deterministic:                                    # train_lm.py:377-381
        torch.backends.cudnn.deterministic = True
        torch.manual_seed(args.local_rank)
    ds = dataset_config(args.dataset_name)
    batch_size = args.batch_size or ds["train_batch_size"]
    log_dir = args.log_dir or ds["checkpoints"]
    device = torch.device("cuda", args.local_rank)
    torch.cuda.set_device(device)
    if getattr(args, "_single_process", False):
        rank, local_rank, world = 0, args.local_rank, 1       # one object per rank: no process group (--objects-across-gpus)
    else:
        rank, local_rank, world = init_distributed("nccl", device)
    if getattr(args, "data", "synthetic") == "rendered":       # batches come from the device as they are: no DataLoader, no sampler
        if world > 1:
            raise SystemExit("-data rendered draws its frames on one device; run it as a single process")
        args.gt_targets = "device"
        loader, sampler = make_rendered(args, "train", args.cls_id, batch_size, device), None
        n_items = len(loader) * batch_size
    else:
        train_ds = make_dataset(args, "train")
        sampler = torch.utils.data.distributed.DistributedSampler(train_ds) if world > 1 else None
        loader = torch.utils.data.DataLoader(train_ds, batch_size=batch_size, shuffle=sampler is None, drop_last=True,
                                             num_workers=4, sampler=sampler)
        n_items = len(train_ds)
    model = build_model(args, args.cls_id).to(device)
    # same update rule as the reference's Adam (train_lm.py:414-416); `fused`: one multi-tensor kernel per step instead of ~25 foreach launches
    optimizer = torch.optim.Adam(model.parameters(), lr=0.0001, weight_decay=args.weight_decay, fused=settings.USE_FUSED_ADAM)
    it, start_epoch = -1, 0
    obj_name = obj_name_of(ds, args.cls_id)
    if args.checkpoint is not None:
        ep = load_checkpoint(model, optimizer, os.path.join(args.checkpoint, obj_name, "geomatch"), device=device, strict=ds["load_strict"])
        if ep is not None:
            start_epoch = ep
    model = wrap_for_training(model, local_rank)
    graphed = None
    if args.graph_train:
        if world > 1:
            raise SystemExit("--graph-train captures a single-process iteration; run multi-rank training without it")
        from .train_graph import GraphedTrainStep
        graphed = GraphedTrainStep(model, optimizer, device,      # before the schedulers: they then drive the device-side lr
                                   gt_targets=getattr(args, "gt_targets", "loader"))
    steps = max(1, args.epochs * n_items // batch_size // 6 // max(world, 1))
    lr_scheduler = torch.optim.lr_scheduler.CyclicLR(optimizer, base_lr=1e-6, max_lr=1e-3, cycle_momentum=False,
                                                     step_size_up=steps, step_size_down=steps, mode="triangular")
    bnm = BNMomentumScheduler(model, lambda i: max(args.bn_momentum * args.bn_decay ** int(i * batch_size / args.decay_step),
                                                   bnm_clip), last_epoch=it)
    trainer = Trainer(model, optimizer, log_dir, obj_name, lr_scheduler, bnm, device,
                      0 if getattr(args, "_single_process", False) else local_rank,     # an objects-across-gpus rank logs / saves its own objects
                      args.save_every, args.log_every, graphed_step=graphed, gt_targets=getattr(args, "gt_targets", "loader"))
    trainer.train(start_epoch, args.epochs, loader, sampler, max_iters=args.max_iters)
    return trainer


def check_dual_flags(args):
    """The -state=test flags of dual-softmax matching, checked against one another: -> whether --match-dual is on."""
    dual = bool(getattr(args, "match_dual", False))
    if dual and getattr(args, "match_gamma", None) is None:
        raise SystemExit("train_lm test: --match-dual needs --match-gamma")
    if getattr(args, "pose_weights", "none") == "dual" and not dual:
        raise SystemExit("train_lm test: --pose-weights dual needs --match-dual")
    if getattr(args, "match_score", "conf") == "dual" and not dual:
        raise SystemExit("train_lm test: --match-score dual needs --match-dual")
    return dual


def test(args):
    """train_lm.py:317-373 without the BOP evaluator: ONE MODEL PER OBJECT of the dataset (:331-340), every batch dispatched per
    instance by its `cls_id` (:298-314) -- grouped per object into true batches here -- then dense matching and the batched GPU
    pose solve (evaluator.py:78-100).  Returns per-batch results in the loader's instance order."""
    rendered = getattr(args, "data", "synthetic") == "rendered"
    verify_names = None
    if getattr(args, "pose_verify", False):
        if not rendered:
            raise SystemExit("train_lm test: --pose-verify needs -data rendered: the other batches carry no depth frame and no mesh "
                             "faces (use pose.verify_poses from Python)")
        verify_names = tuple(k for k in args.verify_candidates.split(",") if k)
        bases = pose.VERIFY_CANDIDATES + ("consensus", "consensus+icp")
        allowed = bases + tuple(k + "+depth" for k in bases)
        if not verify_names or set(verify_names) - set(allowed) or len(set(verify_names)) != len(verify_names):
            raise SystemExit("train_lm test: --verify-candidates takes distinct names out of %s, each optionally followed by +depth, "
                             "got %r" % (", ".join(bases), args.verify_candidates))
        if args.graph_batch1:
            raise SystemExit("train_lm test: --pose-verify does not go with --graph-batch1")
    ds = dataset_config(args.dataset_name)
    batch_size = args.batch_size or ds["val_batch_size"]
    device = torch.device("cuda", args.local_rank)
    torch.cuda.set_device(device)
    ids = [args.cls_id] if args.single_object or rendered else sorted(ds["objs"])
    ckpt_root = args.checkpoint or ds["checkpoints"]
    model_dict = {}
    for cid in ids:
        model = build_model(args, cid, cache_mesh_in_eval=True).to(device)
        stem = os.path.join(ckpt_root, obj_name_of(ds, cid), "geomatch")
        if os.path.exists(stem + ".pth.tar"):                 # the reference also skips objects without a checkpoint (:336)
            load_checkpoint(model, None, stem, device=device, strict=ds["load_strict"])
        model_dict[cid] = model.eval()
    if rendered:
        loader = make_rendered(args, "test", args.cls_id, batch_size, device, keep_frames=verify_names is not None)
    else:
        loader = torch.utils.data.DataLoader(make_dataset(args, "test", cls_ids=ids), batch_size=batch_size, shuffle=False, num_workers=2)
    graphs = {}
    results = []
    pose_kw = dict(pose_fit=args.pose_fit, icp_iters=args.icp_iters,
                   pose_opts=dict(ransac_iters=args.ransac_iters, ransac_inlier_dist=args.ransac_inlier_dist,
                                  consensus_tau=getattr(args, "consensus_tau", 0.005), consensus_seeds=getattr(args, "consensus_seeds", 8),
                                  consensus_inlier_dist=getattr(args, "consensus_inlier_dist", 0.015),
                                  icp_tolerance=args.icp_tolerance))
    if getattr(args, "icp_metric", "point") == "plane":
        pose_kw["pose_opts"].update(icp_metric="plane", icp_huber=args.icp_huber, icp_normal_gate=args.icp_normal_gate)
    elif getattr(args, "icp_huber", None) is not None or getattr(args, "icp_normal_gate", None) is not None:
        raise SystemExit("train_lm test: --icp-huber / --icp-normal-gate go with --icp-metric plane")
    match_gamma = getattr(args, "match_gamma", None)
    match_dual = check_dual_flags(args)
    soft_pose = (getattr(args, "pose_weights", "none"), getattr(args, "pose_targets", "vertex")) != ("none", "vertex")
    if soft_pose and match_gamma is None:
        raise SystemExit("train_lm test: --pose-weights conf / --pose-targets soft need --match-gamma")
    if soft_pose and args.pose_fit != "kabsch":
        raise SystemExit("train_lm test: --pose-weights conf / --pose-targets soft go with --pose-fit kabsch (RANSAC keeps the hard pairs)")
    if soft_pose:
        pose_kw["pose_opts"].update(weights=args.pose_weights, targets=args.pose_targets)
    if match_gamma is not None:
        pose_kw["match_gamma"] = match_gamma
    if match_dual:
        pose_kw["match_dual"] = True
    pair_filter = getattr(args, "pair_filter", "none")
    if pair_filter == "cycle":
        if match_gamma is not None and not match_dual:
            raise SystemExit("train_lm test: --pair-filter cycle does not go with --match-gamma (there is no soft two-way kernel) unless "
                             "--match-dual is given")
        pose_kw["pose_opts"].update(pair_filter="cycle", cycle_radius=pose.CYCLE_RADIUS if getattr(args, "cycle_radius", None) is None
                                    else args.cycle_radius)
    elif getattr(args, "cycle_radius", None) is not None:
        raise SystemExit("train_lm test: --cycle-radius goes with --pair-filter cycle")
    kept = {}                                                # object name -> [kept pairs, masked points] over the run
    # evaluator.py:308-463: when the loader carries ground-truth poses (`RT`), every instance's ADD(-S) / re / te / re-projection error
    # is computed on the device per object group and the reference's recall table is printed at the end
    from . import evaluation
    table = evaluation.RecallTable()
    prec_table = evaluation.RecallTable(precision=True)      # evaluator.py:466-660, written beside the recall table with --eval_output
    bop = evaluation.BopCsv()                                # evaluator.py:341,365-373: one line per predicted instance
    # --bop-scores: MSSD / MSPD (pose_error.py:131-179) over the model points the run already has, against every symmetric copy of
    # the ground truth (misc.py:206-254; models_info.json is in millimetres, the poses in metres).  VSD needs the whole depth frame
    # and the mesh faces, which these batches do not carry: it stays with the Python API (evaluation.vsd_from_poses).
    bop_scores = evaluation.BopScores() if getattr(args, "bop_scores", False) else None
    syms = {}
    if bop_scores is not None:
        info = evaluation.load_models_info(args.models_info) if getattr(args, "models_info", None) else {}
        if not info:
            import warnings
            warnings.warn("train_lm test --bop-scores without --models-info: no object symmetries, MSSD / MSPD against the identity only")
        for cid in ids:
            R, t = evaluation.symmetry_transformations(info.get(cid, {}), scale=0.001)
            syms[cid] = (torch.from_numpy(R).to(device), torch.from_numpy(t).to(device))
    # --pose-verify: the mesh _rendered_meshes drew (metres), the depth frame and the padded box of every item; one recall table per
    # candidate beside the selection's
    verify_mesh, cand_tables = None, {}
    if verify_names is not None:
        mesh = _rendered_meshes(args, args.cls_id)[0][0]
        verify_mesh = (torch.from_numpy(np.asarray(mesh["verts"], dtype=np.float64) / 1000.0).to(device),
                       torch.from_numpy(np.ascontiguousarray(mesh["faces"]).astype(np.int32)).to(device))
        cand_tables = {k: evaluation.RecallTable() for k in verify_names}
    n_seen = 0
    bop_ids_seen = True                                      # every batch so far carried scene_id / im_id
    sym_names = set(ds.get("sym_objs", ()))                 # config/*_cfg.py SYM_OBJS: object NAMES
    with torch.no_grad():
        for batch in loader:
            t0 = time.perf_counter()
            cu = to_device(batch, device)
            cls = cu["cls_id"].cpu().tolist() if "cls_id" in cu else [args.cls_id] * cu["cld_rgb_nrm"].shape[0]
            if args.graph_batch1 and args.model_variant == "ffb6d" and len(cls) == 1:
                cid = cls[0]
                one = {k: cu[k] for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
                if cid not in graphs:
                    graphs[cid] = infer.GraphedPipeline(model_dict[cid], one, **pose_kw)
                out = {k: v.clone() for k, v in graphs[cid](one).items()}
            elif verify_names is not None:
                fd = cu["frame_depth"]
                verify = dict(verts=verify_mesh[0], faces=verify_mesh[1], depth=fd, K=cu["K"], delta=args.verify_delta,
                              window=pose.boxes_to_windows(cu["bbox"], fd.shape[-2], fd.shape[-1]), candidates=verify_names,
                              icp_iters=args.icp_iters or 10, depth_iters=getattr(args, "depth_refine_iters", 5),
                              depth_opts=dict(reject=getattr(args, "depth_refine_reject", 0.01)))
                out = infer.run_multi_object(model_dict, cu, cls, **dict(pose_kw, verify=verify))
                out["score"] = out["verify_score"].float()                 # the csv score
            else:
                out = infer.run_multi_object(model_dict, cu, cls, **pose_kw)
            if getattr(args, "match_score", "conf") == "dual" and verify_names is None:
                out["score"] = ops.match_score(out["dual"], out["mask"])  # the csv score: the mean dual confidence of the masked points
            torch.cuda.synchronize()
            results.append(dict(time=time.perf_counter() - t0, cls_id=cls, count=out["mask"].sum(dim=1).cpu(), best_idx=out["best_idx"].cpu(),
                                best_sim=out["best_sim"].cpu(), mask=out["mask"].cpu(), RT=out["RT"].cpu(), valid=out["valid"].cpu()))
            if verify_names is not None:
                results[-1].update(score=out["score"].cpu(), verify_which=out["verify_which"].cpu(), verify_counts=out["verify_counts"].cpu())
            elif "score" in out:
                results[-1].update(score=out["score"].cpu(), conf=out["conf"].cpu())
            if "dual" in out:
                results[-1].update(dual=out["dual"].cpu())
            if "pair_count" in out:
                results[-1].update(pair_mask=out["pair_mask"].cpu(), pair_count=out["pair_count"].cpu())
                for i, cid in enumerate(cls):
                    k = kept.setdefault(obj_name_of(ds, cid), [0, 0])
                    k[0] += int(results[-1]["pair_count"][i])
                    k[1] += int(results[-1]["count"][i])
            if "RT" in cu and cu["RT"].dim() == 3:
                Kcam = cu["K"] if "K" in cu else torch.from_numpy(synthetic.LM_K).to(device)
                for cid in sorted(set(cls)):
                    rows = torch.tensor([i for i, c in enumerate(cls) if c == cid], device=device)
                    err = evaluation.pose_errors(out["RT"][rows], cu["RT"][rows][:, :3], model_dict[cid].model_emb.xyz,
                                                 Kcam[rows] if Kcam.dim() == 3 else Kcam, symmetric=obj_name_of(ds, cid) in sym_names,
                                                 sym_rots=getattr(model_dict[cid].model_emb, "sym_rots", None))
                    table.update(obj_name_of(ds, cid), err, ds["diameters"][cid] / 1000.0)
                    prec_table.update(obj_name_of(ds, cid), err, ds["diameters"][cid] / 1000.0)
                    for c, name in enumerate(verify_names or ()):
                        cand_tables[name].update(obj_name_of(ds, cid), evaluation.pose_errors(
                            out["verify_cand_RT"][rows][:, c], cu["RT"][rows][:, :3], model_dict[cid].model_emb.xyz,
                            Kcam[rows] if Kcam.dim() == 3 else Kcam, symmetric=obj_name_of(ds, cid) in sym_names,
                            sym_rots=getattr(model_dict[cid].model_emb, "sym_rots", None)), ds["diameters"][cid] / 1000.0)
                    if bop_scores is not None:
                        mssd, mspd, _, _ = evaluation.mssd_mspd(out["RT"][rows], cu["RT"][rows][:, :3], model_dict[cid].model_emb.xyz,
                                                                syms[cid][0], syms[cid][1], Kcam[rows] if Kcam.dim() == 3 else Kcam)
                        bop_scores.update(obj_name_of(ds, cid), mssd, mspd, None, ds["diameters"][cid] / 1000.0,
                                          int(ds.get("image_width", 640)))
            # The reference walks the GROUND-TRUTH annotations (evaluator.py:340-373): a csv line is appended only for a prediction that
            # has a ground-truth entry, keyed by the real "scene/.../im_id" (:366-367), and a ground truth without a prediction counts as a
            # miss in the recall table (:355-363).  So: lines only where the loader supplied RT AND scene_id / im_id (ids invented here
            # would mean nothing to bop_toolkit and change with the batch order -- without them the csv is not written, see below), and
            # `n_undetected` [bs] (ground truths of the instance's object in its image that the detector missed), when the loader
            # carries it, goes to RecallTable.missing.
            has_gt = "RT" in cu and cu["RT"].dim() == 3
            has_ids = "scene_id" in batch and "im_id" in batch
            bop_ids_seen = bop_ids_seen and has_ids
            if has_gt and has_ids:
                for i, cid in enumerate(cls):
                    bop.add("%06d/%06d" % (int(batch["scene_id"][i]), int(batch["im_id"][i])), cid, out["RT"][i, :, :3], out["RT"][i, :, 3],
                            score=float(out["score"][i]) if "score" in out else -1)
            if has_gt and "n_undetected" in batch:
                for i, cid in enumerate(cls):
                    miss = int(batch["n_undetected"][i])
                    if miss > 0:
                        table.missing(obj_name_of(ds, cid), miss)
                        prec_table.missing(obj_name_of(ds, cid), miss)      # (the precision variant ignores them: evaluator.py:549-551)
                        if bop_scores is not None:
                            bop_scores.missing(obj_name_of(ds, cid), miss)
            n_seen += len(cls)
    if table.recalls:
        test.last_table = table
        test.last_candidate_tables = cand_tables
        if args.local_rank == 0:
            for name, t in cand_tables.items():
                print("--pose-verify candidate %s:" % name)
                print(t.format())
            if cand_tables:
                print("--pose-verify selection (delta %g m):" % args.verify_delta)
            print(table.format())
    if kept:
        test.last_kept = kept
        if args.local_rank == 0:
            print("--pair-filter cycle (radius %g m): kept fraction of the masked points" % pose_kw["pose_opts"]["cycle_radius"])
            for name in sorted(kept):
                print("  %-16s %8d / %8d = %.3f" % (name, kept[name][0], kept[name][1], kept[name][0] / max(kept[name][1], 1)))
    if bop_scores is not None and bop_scores.correct:
        test.last_bop_scores = bop_scores
        if args.local_rank == 0:
            print(bop_scores.format())
    if getattr(args, "eval_output", None) and args.local_rank == 0:
        # what the reference's evaluator leaves behind: the BOP result csv (:429-431) and, when ground truth was there, the error /
        # recall pickles and the table text of both variants (:449-455, :647-660)
        written = []
        if bop_ids_seen and len(bop.lines) > 1:
            written.append(bop.write(os.path.join(args.eval_output, "%s_%s-test.csv" % (args.model_variant, args.dataset_name))))
        else:
            import warnings
            warnings.warn("train_lm test: the BOP result csv was NOT written: the dataset does not carry `scene_id` / `im_id` (or no "
                          "instance had a ground-truth pose); the reference keys every csv line by them (evaluator.py:366-373)")
        if table.recalls:
            written += list(table.dump(args.eval_output, args.dataset_name + "_test"))
            written += list(prec_table.dump(args.eval_output, args.dataset_name + "_test", method_name=args.model_variant))
        if bop_scores is not None and bop_scores.correct:
            written += list(bop_scores.dump(args.eval_output, args.dataset_name + "_test", method_name=args.model_variant))
        test.last_outputs = written
    return results


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.gpu is not None:
        os.environ["CUDA_VISIBLE_DEVICES"] = args.gpu
    if args.state == "train":
        train(args)
    else:
        res = test(args)
        print("processed %d batches, %.1f ms/batch" % (len(res), 1e3 * float(np.mean([r["time"] for r in res]))))


if __name__ == "__main__":
    main()
