"""FFB6DEmb: bidirectional fusion of the image branch and the RandLA point branch.

Mirrors /root/reference/models/ffb6d.py:9-285 (constructor layout and parameter names identical,
so `pcd_emb.*` checkpoint keys load unchanged; forward follows :172-285 stage by stage).

HIP operators replace the reference's gather chains:
  random_sample (:128-146)          -> ops.gather_max   (index read once, max over K in registers)
  nearest_interpolation (:148-163)  -> ops.gather_nn
  choose gather (:278-281)          -> ops.gather_nn
Neighbour indices are consumed as int32 (int64 accepted and narrowed).
"""
import collections
import contextlib

import torch
import torch.nn as nn

from . import ops, pyramid, settings
from .cnn import FinalStage, PSPNet, PSPUpsample, bn_act
from .derived import derived
from .layers import act_code, cached_gemm_weight, folded_bn, fused_eval, pt_conv2d, rl_conv1d, rl_conv2d
from .randla import DilatedResBlock


# The forms a point-to-pixel (p2r) fusion site takes.  point_major: the layout of the point term the form reads -- [B, n', C] (True),
# [B, C, n'] (False), no separate term (None); _p2r_point_term produces what this says and the form's executor reads it.
# pixel_major: the form can write its map as [B, H*W, C].
_P2RPath = collections.namedtuple("_P2RPath", "name point_major pixel_major")
MFMA64 = _P2RPath("MFMA64", True, True)         # 64 -> 64 channels on the matrix cores; also the packed output and the fused `final`
FMA64 = _P2RPath("FMA64", False, True)          # the same shapes in exact fp32 FMAs (settings.USE_MFMA_GEMM off)
GEMM = _P2RPath("GEMM", False, False)           # every other channel count: a GEMM, then (or with, as its epilogue) the gather
MODULES = _P2RPath("MODULES", None, False)      # gather, torch.cat and the layer itself: training, and any activation the kernels do not know


def _p2r_path(fuse_layer, c, fused):
    """The form the p2r fusion through `fuse_layer` takes on a c-channel map; fused = fused_eval(...) of the forward.  The ONE place
    this is decided: the point-term producer, _p2r_fuse, _fused_final_stage and _sparse_final_ok all read the returned value."""
    if not fused or act_code(getattr(fuse_layer, "activation", None)) is None:
        return MODULES
    if c == 64 and fuse_layer.conv.weight.shape[0] == 64:
        return MFMA64 if settings.USE_MFMA_GEMM else FMA64
    return GEMM


class _Lanes:
    """The two lanes of FFB6DEmb.forward's stage loop.  The image lane is the current stream; the point lane is side stream 0 when
    `two`, and otherwise the image lane itself -- then exchange() does nothing and point() scopes nothing."""

    def __init__(self, inputs, two):
        dev = inputs["rgb"].device
        self.inputs, self.two = inputs, bool(two)
        self.image = torch.cuda.current_stream(dev) if two else None
        self.side = ops.side_stream(dev, 0) if two else None

    def point(self):
        """with lanes.point(): the body is enqueued on the point lane."""
        return torch.cuda.stream(self.side) if self.two else contextlib.nullcontext()

    def exchange(self, to_point=(), to_image=(), ready=False):
        """Hand `to_point` (made on the image lane) to the point lane and `to_image` the other way.  An event is recorded on each
        producing lane BEFORE either lane waits, so neither event carries the other lane's work; then each consuming lane waits for
        its event, and every tensor that crosses is recorded on the stream that did not allocate it.  ready: both lanes also wait
        for the whole neighbour pyramid (pyramid.wait_ready) before their first use of the indices a RandLA block does not read."""
        if not self.two:
            return
        ev_image = self.image.record_event() if to_point else None
        ev_point = self.side.record_event() if to_image else None
        if to_point:
            self.side.wait_event(ev_image)
            self._keep(to_point, self.side)
        if ready:
            pyramid.wait_ready(self.inputs, self.side)
            pyramid.wait_ready(self.inputs, self.image)
        if to_image:
            self.image.wait_event(ev_point)
            self._keep(to_image, self.image)

    @staticmethod
    def _keep(tensors, lane):
        for t in tensors:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(lane)


class FFB6DEmb(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        cnn = PSPNet()
        d_outs = list(cfg.d_out)
        n_layers = cfg.num_layers

        self.cnn_pre_stages = nn.Sequential(cnn.feats.conv1, cnn.feats.bn1, cnn.feats.relu, cnn.feats.maxpool)
        self.rndla_pre_stages = rl_conv1d(cfg.in_c, 8, bn=True)                  # RandLANet.py:19 fc0

        self.cnn_ds_stages = nn.ModuleList([
            cnn.feats.layer1,
            cnn.feats.layer2,
            nn.Sequential(cnn.feats.layer3, cnn.feats.layer4),
            nn.Sequential(cnn.psp, cnn.drop_1),
        ])
        self.ds_sr = [4, 8, 8, 8]

        blocks = nn.ModuleList()                                                 # RandLANet.py:21-26
        d_in = 8
        for i in range(n_layers):
            blocks.append(DilatedResBlock(d_in, d_outs[i]))
            d_in = 2 * d_outs[i]
        self.rndla_ds_stages = blocks

        self.ds_rgb_oc = [64, 128, 512, 1024]
        self.ds_rndla_oc = [c * 2 for c in d_outs]
        self.ds_fuse_r2p_pre_layers = nn.ModuleList()
        self.ds_fuse_r2p_fuse_layers = nn.ModuleList()
        self.ds_fuse_p2r_pre_layers = nn.ModuleList()
        self.ds_fuse_p2r_fuse_layers = nn.ModuleList()
        for i in range(4):
            self.ds_fuse_r2p_pre_layers.append(pt_conv2d(self.ds_rgb_oc[i], self.ds_rndla_oc[i], bn=True))
            self.ds_fuse_r2p_fuse_layers.append(pt_conv2d(self.ds_rndla_oc[i] * 2, self.ds_rndla_oc[i], bn=True))
            self.ds_fuse_p2r_pre_layers.append(pt_conv2d(self.ds_rndla_oc[i], self.ds_rgb_oc[i], bn=True))
            self.ds_fuse_p2r_fuse_layers.append(pt_conv2d(self.ds_rgb_oc[i] * 2, self.ds_rgb_oc[i], bn=True))

        self.cnn_up_stages = nn.ModuleList([
            nn.Sequential(cnn.up_1, cnn.drop_2),
            nn.Sequential(cnn.up_2, cnn.drop_2),
            nn.Sequential(cnn.final),
            nn.Sequential(cnn.up_3, cnn.final),              # `final` is shared, as in the reference (:79-80)
        ])
        self.up_rgb_oc = [256, 64, 64]
        self.up_rndla_oc = []
        for j in range(n_layers):
            self.up_rndla_oc.append(self.ds_rndla_oc[-j - 2] if j < 3 else self.ds_rndla_oc[0])

        dec = nn.ModuleList()                                                    # RandLANet.py:28-39 decoder_blocks
        d_out = 2 * d_outs[-1]
        for j in range(n_layers):
            if j < 3:
                d_in = d_out + 2 * d_outs[-j - 2]
                d_out = 2 * d_outs[-j - 2]
            else:
                d_in = 4 * d_outs[-4]
                d_out = 2 * d_outs[-4]
            dec.append(rl_conv2d(d_in, d_out, bn=True))
        self.rndla_up_stages = dec

        self.up_fuse_r2p_pre_layers = nn.ModuleList()
        self.up_fuse_r2p_fuse_layers = nn.ModuleList()
        self.up_fuse_p2r_pre_layers = nn.ModuleList()
        self.up_fuse_p2r_fuse_layers = nn.ModuleList()
        for i in range(3):
            self.up_fuse_r2p_pre_layers.append(pt_conv2d(self.up_rgb_oc[i], self.up_rndla_oc[i], bn=True))
            self.up_fuse_r2p_fuse_layers.append(pt_conv2d(self.up_rndla_oc[i] * 2, self.up_rndla_oc[i], bn=True))
            self.up_fuse_p2r_pre_layers.append(pt_conv2d(self.up_rndla_oc[i], self.up_rgb_oc[i], bn=True))
            self.up_fuse_p2r_fuse_layers.append(pt_conv2d(self.up_rgb_oc[i] * 2, self.up_rgb_oc[i], bn=True))

    # same names and contracts as the reference's static methods (ffb6d.py:128-163)
    @staticmethod
    def random_sample(feature, pool_idx):
        return ops.gather_max(feature, pool_idx).unsqueeze(3)

    @staticmethod
    def nearest_interpolation(feature, interp_idx):
        return ops.gather_nn(feature, interp_idx).unsqueeze(3)

    @staticmethod
    def _split_fuse_weight(layer, c_first):
        """1x1 fuse conv over cat(a, b): W = [W_a | W_b] split at channel c_first (contiguous copies, cached)."""
        w = layer.conv.weight

        def make():
            w2 = w.view(w.shape[0], -1)
            return w2[:, :c_first].contiguous(), w2[:, c_first:].contiguous()
        return derived(layer, "split", (w,), make, extra=(c_first,))

    @staticmethod
    def _fuse_weight_t(layer, wa, tag="a"):
        """wa transposed ([ci][co], contiguous), cached beside the split weights."""
        return derived(layer, "w%s_t" % tag, (wa,), lambda: wa.t().contiguous())

    def _p2r_point_term(self, path, pre_layer, fuse_layer, split, p_emb0):
        """The point half of the p2r fusion, W_b . pre(p_emb0), at the points (a 1x1 conv commutes with the gather), in the layout
        `path` reads: [B, n', 64] where path.point_major, else [B, Cout, n']; None for MODULES, which has no separate term.  The one
        producer of the term: the stage loop forms it on the point lane, so the image lane only waits for the finished term.
        split = _split_fuse_weight(fuse_layer, c), which the stage loop looks up once for this and for _p2r_fuse."""
        if path is MODULES:
            return None
        wb = split[1]
        pp = pre_layer(p_emb0).reshape(p_emb0.shape[0], wb.shape[1], -1)
        if settings.USE_POINTWISE:
            return ops.pointwise([pp], self._fuse_weight_t(fuse_layer, wb, "b"), point_major=path.point_major)
        return torch.matmul(pp.transpose(1, 2), wb.t()) if path.point_major else ops.wx(wb, pp)

    def _p2r_fuse(self, path, pre_layer, fuse_layer, split, rgb_emb0, p_emb0, term, idx, pixel_major=False, want_packed=False,
                  packed_only=False, final=None):
        """fuse(cat(rgb_emb0, nearest_interp(pre(p_emb0)))) (ffb6d.py:216-222,252-258) in the form `path` names (_p2r_path), with
        `term` from _p2r_point_term(path, ...) and the same `split` (W_a, W_b).  Eval: the pixel half of the 1x1 fuse convolution is a
        GEMM with half the K, and gather + add + BN + ReLU is one HIP launch; no concat, no full-resolution point features.
        packed_only (the caller's promise, _packed_only_consumer): the next image stage reads the packed operand and nothing else, so
        GEMM returns the ops.PackedAct alone and the fp32 map is never stored.  final (_fused_final_stage): the FinalStage that is the
        fused map's only reader; MFMA64 then returns final(fused map) from one launch, the map never stored."""
        if (pixel_major and not path.pixel_major) or (final is not None and path is not MFMA64):
            raise RuntimeError("pixel-major output is the 64-channel kernels', the fused `final` MFMA64's, and this fusion takes %s; "
                               "_sparse_final_ok() and _fused_final_stage() guard the caller" % path.name)
        if path is MODULES:
            bs, _, hr, wr = rgb_emb0.shape
            p2r_emb = self.nearest_interpolation(pre_layer(p_emb0), idx).view(bs, -1, hr, wr)
            return fuse_layer(torch.cat((rgb_emb0, p2r_emb), dim=1))
        code = act_code(getattr(fuse_layer, "activation", None))
        if path is MFMA64:
            return self._fuse_mfma64(fuse_layer, split[0], rgb_emb0, term, idx, code, pixel_major, want_packed, final)
        if path is FMA64:
            return self._fuse_fma64(fuse_layer, split[0], rgb_emb0, term, idx, code, pixel_major)
        return self._fuse_gemm(fuse_layer, split[0], rgb_emb0, term, idx, code, packed_only)

    def _fuse_mfma64(self, fuse_layer, wa, rgb_emb0, t_pm, idx, code, pixel_major, want_packed, final):
        """K = 64: channel mix on the matrix cores (split-bf16 x3) + gather + add + BN + ReLU in ONE pass over the pixels, bound by the
        map's read + write; the point term is point-major ([B, n', 64]: one contiguous row per gathered point)."""
        bs, c, hr, wr = rgb_emb0.shape
        scale, shift = folded_bn(fuse_layer.normlayer.bn)
        wa_pk = derived(fuse_layer, "wa_pk", (wa,), lambda: ops.pack_rows64(wa))
        if final is not None:
            fconv = final[0]
            return ops.conv64_gather_add_final(rgb_emb0.reshape(bs, c, hr * wr), wa_pk, t_pm, idx.reshape(bs, -1), scale, shift,
                                               code[0], code[1], fconv.weight, fconv.bias).view(bs, -1, hr, wr)
        y = ops.conv64_gather_add_act_mfma(rgb_emb0.reshape(bs, c, hr * wr), wa_pk, t_pm, idx.reshape(bs, -1), scale, shift,
                                           code[0], code[1], pixel_major=pixel_major, t_point_major=MFMA64.point_major,
                                           hw=(hr, wr) if (want_packed and settings.USE_PACKED_PRODUCERS and not pixel_major) else None)
        if pixel_major:
            return y                                    # [B, H*W, 64] for _final_at_choose
        # the next stage's first convolution reads the operand the kernel wrote (of the [B, 64, H, W] map): no pack launch
        return ops.carry_packed(y.view(bs, -1, hr, wr), ops.packed_of(y, (bs, c, hr, wr)))

    def _fuse_fma64(self, fuse_layer, wa, rgb_emb0, t, idx, code, pixel_major):
        """K = 64: GEMM + gather + add + BN + ReLU in ONE pass over the pixels (exact fp32 FMAs); channel-major point term."""
        bs, c, hr, wr = rgb_emb0.shape
        scale, shift = folded_bn(fuse_layer.normlayer.bn)
        y = ops.conv1x1_gather_add_act(rgb_emb0.reshape(bs, c, hr * wr), self._fuse_weight_t(fuse_layer, wa), t,
                                       idx.reshape(bs, -1), scale, shift, code[0], code[1], pixel_major=pixel_major)
        return y if pixel_major else y.view(bs, -1, hr, wr)  # pixel-major: [B, H*W, 64] for _final_at_choose

    def _fuse_gemm(self, fuse_layer, wa, rgb_emb0, t, idx, code, packed_only):
        """Every other channel count: the pixel half as a GEMM, then gather + add + BN + activation (channel-major point term).  Which
        GEMM depends on the operand the map carries at run time, so that choice is made here."""
        bs, c, hr, wr = rgb_emb0.shape
        if settings.USE_MFMA_GEMM and ops.gemm_supported(c, wa.shape[0], hr * wr, bs):
            wpk, co = cached_gemm_weight(fuse_layer, "wa", wa, (fuse_layer.conv.weight,))
            only = packed_only and ops.packed_out_supported(bs, co, hr, wr)
            if ops.conv1x1_gather_add_supported(rgb_emb0, co, code[0], f32_out=not only):
                # the GEMM runs inside gather_add_affine_act's launch (ops.conv1x1_packed_gather_add_act): gather, add, BN and
                # activation are its epilogue, the fp32 map between the two is never written
                x = ops.GemmMap(rgb_emb0, wpk, co)
            else:
                x = ops.gemm_bf16x3_map(rgb_emb0, wpk, co).view(bs, co, hr * wr)   # split-bf16 MFMA; reads the stage's packed output
        else:
            x = ops.wx(wa, rgb_emb0.reshape(bs, c, hr * wr))                    # [B,Cout,HW]
        scale, shift = folded_bn(fuse_layer.normlayer.bn)
        if packed_only and ops.packed_out_supported(bs, x.shape[1], hr, wr):
            return ops.gather_add_affine_act(x, t, idx.reshape(bs, -1), scale, shift, code[0], code[1], hw=(hr, wr), f32_out=False)
        y, ypk = ops.gather_add_affine_act(x, t, idx.reshape(bs, -1), scale, shift, code[0], code[1], hw=(hr, wr))
        return ops.carry_packed(y.view(bs, -1, hr, wr), ypk)   # the next image stage's first convolution / GEMM reads this: no pack launch

    def _packed_only_consumer(self, stage, shape):
        """True when image stage `stage`, given a GPU map of this shape, reads its packed operand and nothing else: Sequential(PSPUpsample,
        dropout) in eval (the dropout is the identity) whose up-sampling stage takes its tap GEMM on the packed operand."""
        return (isinstance(stage, nn.Sequential) and len(stage) == 2 and isinstance(stage[0], PSPUpsample)
                and isinstance(stage[1], (nn.Dropout, nn.Dropout2d)) and not stage[1].training and stage[0].reads_packed_only(shape))

    @staticmethod
    def _image_stage(stage, x):
        """stage(x); a packed-only map (see _packed_only_consumer) goes straight to the up-sampling stage, past the identity dropout."""
        return stage[0](x) if isinstance(x, ops.PackedAct) else stage(x)

    def _fused_final_stage(self, i_up, path, batch, pixel_major):
        """The FinalStage that _p2r_fuse of up stage i_up may apply in the same launch, or None: the fusion is MFMA64 in NCHW form, and
        the next image stage is `final` alone, 64 -> 64, so the fused map has no other reader (the r2p gather of that stage reads
        rgb_emb0, the following stage reads final's output)."""
        if pixel_major or i_up + 1 >= len(self.rndla_up_stages) - 1 or path is not MFMA64 or batch > 65535:
            return None
        nxt = self.cnn_up_stages[i_up + 1]
        if not (isinstance(nxt, nn.Sequential) and len(nxt) == 1 and isinstance(nxt[0], FinalStage) and not nxt[0].training):
            return None
        fconv = nxt[0][0]
        if not (isinstance(fconv, nn.Conv2d) and fconv.in_channels == 64 and fconv.out_channels == 64 and fconv.kernel_size == (1, 1)):
            return None
        return nxt[0]

    def forward(self, inputs, end_points=None, parts=False):
        """-> f32[B,128,N] (ffb6d.py:285: cat of the 64 image channels at the chosen pixels and the 64 point channels); parts=True
        returns the two halves un-concatenated, for a consumer that reads them in place (the fused per-point heads).

        The seven stages run against two lanes (_Lanes): the IMAGE lane (the current stream) runs the trunk / up stages and the
        point-to-pixel fusions, the POINT lane the RandLA blocks, the decoder layers, the point terms and the pixel-to-point fusions.
        Inference with settings.USE_SIDE_STREAMS and "point" in SIDE_PARTS puts the point lane on side stream 0: per stage each stream
        waits ONCE for the other's product (the point stream for the image stage's map `rgb_emb0`, read by the r2p gather; the image
        stream for `p_emb0` and the point term, read by the p2r fusion) and otherwise they run ahead independently -- the r2p chain of
        stage i and the RandLA block of stage i + 1 sit in the shadow of the convolutions of stage i + 1.  Everything else (training
        too) runs the same loop with both lanes on the current stream: the same kernels on the same operands in the same enqueue
        order, bit-identical (tests/test_gpu_headline.py::test_timed_configuration_bit_exact_across_launch_forms)."""
        fused = fused_eval(inputs["rgb"], self)
        if fused:
            pre = self.cnn_pre_stages                                         # conv1, bn1, relu, maxpool
            s0, b0 = folded_bn(pre[1])
            mp = pre[3]
            conv = pre[0]
            plain_pool = (isinstance(mp, nn.MaxPool2d) and mp.kernel_size in (3, (3, 3)) and mp.stride in (2, (2, 2)) and mp.padding in (1, (1, 1))
                          and mp.dilation in (1, (1, 1)) and not mp.ceil_mode and isinstance(pre[2], nn.ReLU))
            if (settings.USE_OWN_STEM and plain_pool and tuple(conv.weight.shape) == (64, 3, 7, 7) and conv.bias is None
                    and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (3, 3) and tuple(conv.dilation) == (1, 1)
                    and inputs["rgb"].shape[0] <= 65535):
                # the whole stem in one own launch (split-bf16 MFMA implicit GEMM, pooled in LDS): no library kernel is left in the step
                rgb_emb = ops.stem(inputs["rgb"], derived(conv, "stem_pk", (conv.weight,), lambda: ops.stem_pack_weight(conv.weight)), s0, b0)
            else:
                y0 = conv(inputs["rgb"])
                if plain_pool and y0.shape[0] * y0.shape[1] <= 65535:
                    rgb_emb = ops.affine_relu_maxpool(y0, s0, b0)          # BN + ReLU + max-pool: one pass over the stem's map
                else:
                    rgb_emb = mp(ops.affine_act(y0, s0, b0, ops.ACT_RELU))
        else:
            pre = self.cnn_pre_stages
            rgb_emb = pre[3](bn_act(pre[1], pre[0](inputs["rgb"]), pre[2]))
        # An overlapped neighbour-pyramid build (pyramid.build_pyramid(..., overlap=True)) is waited for by EACH consuming stream before
        # its first index use: here by the point lane for the cloud's searches (all of it when there is one lane), the rest in stage 0
        lanes = _Lanes(inputs, fused and settings.USE_SIDE_STREAMS and "point" in settings.SIDE_PARTS)
        lanes.exchange(to_point=(inputs["cld_rgb_nrm"],))
        with lanes.point():
            pyramid.wait_ready(inputs, cloud_only=lanes.two)
            p_emb, f_pc0 = self._stem_and_mlp1(inputs["cld_rgb_nrm"])         # [B,8,N,1] (+ the first block's mlp1 of it)

        ds_emb = []
        for i_ds in range(4):
            pre, fuse = self.ds_fuse_p2r_pre_layers[i_ds], self.ds_fuse_p2r_fuse_layers[i_ds]
            rgb_emb0 = self.cnn_ds_stages[i_ds](rgb_emb)
            bs, c, hr, wr = rgb_emb0.size()
            path = _p2r_path(fuse, c, fused)
            split = self._split_fuse_weight(fuse, c) if path is not MODULES else None
            with lanes.point():
                f_encoder_i = self.rndla_ds_stages[i_ds](p_emb, inputs["cld_xyz%d" % i_ds], inputs["cld_nei_idx%d" % i_ds],
                                                         f_pc=f_pc0 if i_ds == 0 else None)
                p_emb0 = self.random_sample(f_encoder_i, inputs["cld_sub_idx%d" % i_ds])
                term = self._p2r_point_term(path, pre, fuse, split, p_emb0)
            lanes.exchange(to_point=(rgb_emb0,), to_image=(p_emb0, term), ready=i_ds == 0)
            with lanes.point():
                r2p_emb = self.random_sample(rgb_emb0.reshape(bs, c, hr * wr), inputs["r2p_ds_nei_idx%d" % i_ds])
                r2p_emb = self.ds_fuse_r2p_pre_layers[i_ds](r2p_emb)
                p_emb = self.ds_fuse_r2p_fuse_layers[i_ds].forward_segs([p_emb0, r2p_emb])       # over cat(p_emb0, r2p_emb), never formed
            ds_emb += [f_encoder_i, p_emb] if i_ds == 0 else [p_emb]
            rgb_emb = self._p2r_fuse(path, pre, fuse, split, rgb_emb0, p_emb0, term, inputs["p2r_ds_nei_idx%d" % i_ds], want_packed=True,
                                     packed_only=i_ds == 3 and self._packed_only_consumer(self.cnn_up_stages[0], rgb_emb0.shape))

        n_up = len(self.rndla_up_stages)
        pm = final_done = False
        for i_up in range(n_up - 1):
            pre, fuse = self.up_fuse_p2r_pre_layers[i_up], self.up_fuse_p2r_fuse_layers[i_up]
            rgb_emb0 = rgb_emb if final_done else self._image_stage(self.cnn_up_stages[i_up], rgb_emb)   # `final` ran inside the last fusion
            bs, c, hr, wr = rgb_emb0.size()
            path = _p2r_path(fuse, c, fused)
            split = self._split_fuse_weight(fuse, c) if path is not MODULES else None
            pm = i_up == n_up - 2 and self._sparse_final_ok(path, bs)         # the last fusion writes pixel-major for _final_at_choose
            final = self._fused_final_stage(i_up, path, bs, pm)
            final_done = final is not None
            with lanes.point():
                # decoder layer over cat(skip, nearest_interpolation(p_emb)): the interpolation is the second segment's index
                p_emb0 = self.rndla_up_stages[i_up].forward_segs([ds_emb[-i_up - 2], (p_emb, inputs["cld_interp_idx%d" % (n_up - i_up - 1)])])
                term = self._p2r_point_term(path, pre, fuse, split, p_emb0)
            lanes.exchange(to_point=(rgb_emb0,), to_image=(p_emb0, term))
            with lanes.point():
                r2p_emb = self.random_sample(rgb_emb0.reshape(bs, c, hr * wr), inputs["r2p_up_nei_idx%d" % i_up])
                r2p_emb = self.up_fuse_r2p_pre_layers[i_up](r2p_emb)
                p_emb = self.up_fuse_r2p_fuse_layers[i_up].forward_segs([p_emb0, r2p_emb])
            rgb_emb = self._p2r_fuse(path, pre, fuse, split, rgb_emb0, p_emb0, term, inputs["p2r_up_nei_idx%d" % i_up], pixel_major=pm, final=final,
                                     packed_only=i_up + 1 < n_up - 1 and self._packed_only_consumer(self.cnn_up_stages[i_up + 1], rgb_emb0.shape))

        with lanes.point():
            p_emb = self.rndla_up_stages[n_up - 1].forward_segs([ds_emb[0], (p_emb, inputs["cld_interp_idx0"])]).squeeze(-1)
        last = self.cnn_up_stages[n_up - 1]
        if pm:
            # the last stage (up_3 + final) is a per-pixel function of a 3x3 neighbourhood and only the N `choose` pixels of its
            # full-resolution output are kept (reference ffb6d.py:266-285): evaluate it there, on the pixel-major fused map
            rgb_emb_c = self._final_at_choose(rgb_emb, (hr, wr), inputs["choose"])
        else:
            # up_3 needs the whole map (in training: its BatchNorm statistics), but FinalStage -- 1x1 convolution + LogSoftmax over
            # channels -- is a per-pixel function, so it commutes with the `choose` gather (reference ffb6d.py:266-285 applies it to all
            # H*W pixels and keeps N): gathered first, forward and backward of the stage touch N pixels, not H*W
            gathered = self._gathered_final_ok()
            rgb_emb = last[0](rgb_emb) if gathered else last(rgb_emb)
            bs, di, _, _ = rgb_emb.size()
            rgb_emb_c = ops.gather_nn(rgb_emb.view(bs, di, -1), inputs["choose"].reshape(bs, -1, 1))
            if gathered:
                rgb_emb_c = last[1](rgb_emb_c.unsqueeze(-1)).squeeze(-1)
        lanes.exchange(to_image=(p_emb,))
        if parts:
            return rgb_emb_c, p_emb
        return torch.cat([rgb_emb_c, p_emb], dim=1)

    def _stem_and_mlp1(self, x):
        """The RandLA stem fc0 (RandLANet.py:19) and the first block's mlp1 (:683) as ONE launch of two chained per-point layers
        (settings.USE_POINT_CHAIN; same sums in the same order as the two launches) -> (p_emb [B,8,N,1], mlp1(p_emb) [B,16,N,1] or None)."""
        blk = self.rndla_ds_stages[0]
        if settings.USE_POINT_CHAIN and settings.USE_POINTWISE and fused_eval(x, self) and x.dim() == 3:
            p0, p1 = self.rndla_pre_stages._pointwise_params(), blk.mlp1._pointwise_params()
            if (p0 is not None and p1 is not None and p0[0].shape[0] <= 16 and p0[0].shape[1] <= 16 and p1[0].shape[1] <= 32
                    and p1[0].shape[0] == p0[0].shape[1]):
                y0, y1 = ops.pointwise_chain2(x, p0, p1)
                return y0.unsqueeze(3), y1.unsqueeze(3)
        return self.rndla_pre_stages(x).unsqueeze(3), None

    def _gathered_final_ok(self):
        last = self.cnn_up_stages[len(self.rndla_up_stages) - 1]
        return settings.USE_GATHERED_FINAL and len(last) == 2 and isinstance(last[1], FinalStage)

    def _sparse_final_ok(self, path, batch):
        """Inference with folded BatchNorm, the last stage = PSPUpsample(64 -> 64) + FinalStage(64 -> 64) and the last fusion (`path`)
        on a 64-channel kernel: then the stage runs at the chosen pixels only."""
        last = self.cnn_up_stages[len(self.rndla_up_stages) - 1]
        if not (settings.USE_SPARSE_FINAL and settings.USE_FUSED_UPCONV and path in (MFMA64, FMA64) and len(last) == 2):
            return False
        up, fin = last[0], last[1]
        if not (isinstance(up, PSPUpsample) and isinstance(fin, FinalStage)):
            return False
        conv, fconv = up.conv[1], fin[0]
        return (conv.in_channels == 64 and conv.out_channels == 64 and fconv.in_channels == 64 and fconv.out_channels == 64
                and act_code(up.conv[3]) is not None and batch <= 65535)

    def _final_at_choose(self, x_pm, hw, choose):
        last = self.cnn_up_stages[len(self.rndla_up_stages) - 1]
        up, fin = last[0], last[1]
        conv, fconv = up.conv[1], fin[0]
        wpk, fpk = derived(self, "final_pk", (conv.weight, fconv.weight),
                           lambda: (ops.upconv_fused64_pack_weight(conv.weight), ops.pack_rows64(fconv.weight.reshape(64, 64))))
        scale, shift = folded_bn(up.conv[2], conv.bias)
        code = act_code(up.conv[3])
        return ops.upconv_final_points(x_pm, hw, choose, wpk, scale, shift, code[0], code[1], fpk, fconv.bias,
                                       (hw[0] * 2, hw[1] * 2))
