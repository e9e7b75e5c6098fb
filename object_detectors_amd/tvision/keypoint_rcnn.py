"""`KeypointRCNN` / `keypointrcnn_resnet50_fpn` and the keypoint branch of `RoIHeads.forward` (tvision/roi_heads.py:186-379,891-932) over
the MI355X kernels.

    model = keypointrcnn_resnet50_fpn(num_classes=2, num_keypoints=17)
    losses = model(images, targets)     # + 'loss_keypoint'; targets[i]['keypoints'] = float32 [G_i, K, 3] (x, y, v); backward already done
    detections = model(images)          # eval: [{'boxes','labels','scores','keypoints' [D, K, 3], 'keypoints_scores' [D, K]}]

Sources.  The rules of the branch - keypoints_to_heatmap, keypointrcnn_loss, heatmaps_to_keypoints, keypointrcnn_inference, resize_keypoints,
_flip_coco_person_keypoints - are the reference's functions, recorded in tests/golden/g18_keypoint_rcnn.npz.  The reference does NOT contain
torchvision's keypoint_rcnn.py; the constructor defaults (min_size (640, ..., 800), max_size 1333, num_classes 2, 17 keypoints), the module
names (keypoint_head.{0,2,..,14}, keypoint_predictor.kps_score_lowres), the layer shapes (8 x Conv2d(3x3, 512) + ReLU,
ConvTranspose2d(512, K, 4, stride 2, padding 1), bilinear x2 with align_corners=False) and the initialisation (kaiming_normal_ fan_out /
relu, zero bias) are written FROM MEMORY of torchvision, which is not installed here either.

Everything of Faster R-CNN (tvision/frcnn.py) is inherited unchanged; the keypoint branch runs as
  * keypoint_roi_pool     MultiScaleRoIAlign(['0'..'3'], 14, 2) into bf16 NHWC [R, 14, 14, 256]: mi355det_mask_roi_pool, as the mask branch;
  * keypoint_head         8 x Conv2d(3x3, pad 1) + ReLU, 256 -> 512 -> ... -> 512: mi355det_conv_fwd_ex (bias + ReLU), mi355det_conv_dgrad_mask,
                          mi355det_conv_wgrad - the MFMA kernels of the backbone, no new convolution kernel;
  * kps_score_lowres      ConvTranspose2d(512, K, 4, 2, 1) as a SUB-PIXEL convolution on the same kernels: a 3x3 / padding 1 convolution
                          512 -> 4 * KP channels (KP = K rounded up to 32) with fp32 output, channel (2a + b) * KP + k = output pixel
                          (2i + a, 2j + b); tap (dy, dx) in {-1, 0, 1}^2 of phase (a, b) holds w[:, k, a + 1 - 2dy, b + 1 - 2dx] where both
                          kernel indices fall in 0..3 (four live taps per phase), zero elsewhere.  Every w[:, k, ky, kx] lives in exactly
                          one (phase, tap), so its weight gradient is a gather out of conv_wgrad's result, no sum;
  * bilinear x2 + keypointrcnn_loss   one fused kernel (mi355det_keypoint_loss): the [R, K, 56, 56] logits are never stored in training;
  * keypoints_to_heatmap              mi355det_keypoint_targets (all images, one launch; the valid count stays on the device);
  * keypointrcnn_inference            mi355det_keypoint_heatmaps + mi355det_heatmaps_to_keypoints: one launch each for all detections
                                      (the reference: two host reads, one bicubic interpolate and one argmax PER RoI).

Row buckets as in tvision/mask_rcnn.py: rows = MASK_BUCKET * ceil(R / MASK_BUCKET); padded rows repeat RoI 0, are not valid for the loss and
receive zero gradient.  The row count comes from the sampler's host counts: the branch adds no host read to the Faster R-CNN step.
Parameters are ordinary fp32 torch parameters (state-dict keys roi_heads.keypoint_head.{0,2,...,14}.*,
roi_heads.keypoint_predictor.kps_score_lowres.*); gradients land in their .grad (head_parameters()).
"""
import torch
from torch import nn

from .. import ops
from .frcnn import FasterRCNN
from .mask_rcnn import MASK_BUCKET, _Packed, _acc_grad, _rows_for
from .roi_align import MultiScaleRoIAlign

# ConvTranspose2d(4, 2, 1) as 3x3 phases: kernel row ky is the tap dy = _TAP[ky] - 1 of phase a = _PHASE[ky] (ky = a + 1 - 2 dy)
_PHASE = (1, 0, 1, 0)
_TAP = (2, 1, 1, 0)


def padded_keypoints(num_keypoints):
    return ops.pad_to(num_keypoints, 32)


def subpixel_weight(w, kp=None):
    """ConvTranspose2d weight [Cin, K, 4, 4] -> the 3x3 convolution weight [4 * KP, Cin, 3, 3] of the sub-pixel form."""
    cin, k = w.shape[0], w.shape[1]
    kp = kp or padded_keypoints(k)
    a = torch.tensor(_PHASE, device=w.device)
    t = torch.tensor(_TAP, device=w.device)
    w3 = w.new_zeros((2, 2, kp, cin, 3, 3))
    w3[a[:, None], a[None, :], :k, :, t[:, None], t[None, :]] = w.permute(2, 3, 1, 0)
    return w3.reshape(4 * kp, cin, 3, 3)


def subpixel_bias(b, kp=None):
    kp = kp or padded_keypoints(b.shape[0])
    b3 = b.new_zeros((4, kp))
    b3[:, :b.shape[0]] = b
    return b3.reshape(-1)


def subpixel_weight_grad(dw3, cin, k):
    """conv_wgrad's result [4 * KP, 3, 3, Cin] of the sub-pixel convolution -> the ConvTranspose2d weight gradient [Cin, K, 4, 4]."""
    kp = dw3.shape[0] // 4
    a = torch.tensor(_PHASE, device=dw3.device)
    t = torch.tensor(_TAP, device=dw3.device)
    g = dw3.reshape(2, 2, kp, 3, 3, cin)[a[:, None], a[None, :], :, t[:, None], t[None, :], :]        # [ky, kx, KP, Cin]
    return g[:, :, :k].permute(3, 2, 0, 1).contiguous()


def depth_to_space(z, k):
    """sub-pixel [R, 14, 14, 4 * KP] -> NCHW [R, K, 28, 28]."""
    r, kp = z.shape[0], z.shape[3] // 4
    return z.reshape(r, 14, 14, 2, 2, kp)[..., :k].permute(0, 5, 1, 3, 2, 4).reshape(r, k, 28, 28)


class KeypointRCNNHeads(nn.Sequential):
    """torchvision's KeypointRCNNHeads (from memory): Conv2d(3x3, padding 1) + ReLU per layer, kaiming_normal_(fan_out, relu), zero bias.
    The Conv2d modules hold the parameters; the computation is KeypointRCNN._kp_forward / _kp_backward."""

    def __init__(self, in_channels, layers):
        if in_channels != 256 or tuple(layers) != (512,) * 8:
            raise NotImplementedError("KeypointRCNNHeads: the HIP path covers 256 input channels and eight 512-channel layers (torchvision's default)")
        d = []
        nxt = in_channels
        for f in layers:
            d.append(nn.Conv2d(nxt, f, 3, stride=1, padding=1))
            d.append(nn.ReLU(inplace=True))
            nxt = f
        super().__init__(*d)
        for m in self.children():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                nn.init.constant_(m.bias, 0)
        self.convs = [m for m in self.children() if isinstance(m, nn.Conv2d)]
        self._packs = [_Packed(lambda w, b: (w, b), ops.conv_shape(MASK_BUCKET, 14, 14, c.in_channels, 512, 3, 1)) for c in self.convs]

    def forward(self, x):
        raise RuntimeError("KeypointRCNNHeads runs inside KeypointRCNN (HIP kernels); there is no eager forward")


class KeypointRCNNPredictor(nn.Module):
    """torchvision's KeypointRCNNPredictor (from memory): kps_score_lowres = ConvTranspose2d(in, K, 4, stride 2, padding 1), then
    F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)."""

    def __init__(self, in_channels, num_keypoints):
        super().__init__()
        if in_channels != 512:
            raise NotImplementedError("KeypointRCNNPredictor: the HIP path covers in_channels = 512 (torchvision's default)")
        self.kps_score_lowres = nn.ConvTranspose2d(in_channels, num_keypoints, 4, stride=2, padding=1)
        nn.init.kaiming_normal_(self.kps_score_lowres.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.kps_score_lowres.bias, 0)
        self.up_scale = 2
        self.num_keypoints = num_keypoints
        self.kp = padded_keypoints(num_keypoints)
        shape = ops.conv_shape(MASK_BUCKET, 14, 14, 512, 4 * self.kp, 3, 1)
        self._pack = _Packed(lambda w, b: (subpixel_weight(w, self.kp), subpixel_bias(b, self.kp)), shape)

    def forward(self, x):
        raise RuntimeError("KeypointRCNNPredictor runs inside KeypointRCNN (HIP kernels); there is no eager forward")


class KeypointRCNN(FasterRCNN):
    """torchvision's KeypointRCNN (constructor from memory) over tvision/frcnn.py:FasterRCNN; **kw are FasterRCNN's arguments, the box
    classifier's long-tail baselines loss_type='seesaw' | 'eql' with eql_tail= among them."""

    def __init__(self, num_classes=2, trainable_backbone_layers=3, tfidf=None, num_keypoints=17, keypoint_roi_pool=None, keypoint_head=None,
                 keypoint_predictor=None, min_size=(640, 672, 704, 736, 768, 800), max_size=1333, **kw):
        super().__init__(num_classes, trainable_backbone_layers, tfidf=tfidf, min_size=min_size, max_size=max_size, **kw)
        self.transform.keypoints = True         # `ingest` takes targets with keypoints for this model
        dev = self.engine.device
        if keypoint_roi_pool is not None and (not isinstance(keypoint_roi_pool, MultiScaleRoIAlign) or keypoint_roi_pool.output_size != (14, 14)):
            raise NotImplementedError("KeypointRCNN: keypoint_roi_pool must be a 14x14 MultiScaleRoIAlign")
        if keypoint_predictor is not None and num_keypoints not in (None, keypoint_predictor.num_keypoints):
            raise ValueError("num_keypoints should be None (or the predictor's own) when keypoint_predictor is specified")
        if keypoint_predictor is None and num_keypoints is None:
            num_keypoints = 17
        self.keypoint_roi_pool = keypoint_roi_pool or MultiScaleRoIAlign(["0", "1", "2", "3"], 14, 2)
        self.keypoint_head = (keypoint_head or KeypointRCNNHeads(256, (512,) * 8)).to(dev)
        self.keypoint_predictor = (keypoint_predictor or KeypointRCNNPredictor(512, num_keypoints)).to(dev)
        self.num_keypoints = self.keypoint_predictor.num_keypoints
        self.last_keypoint_rows = None
        self.keep_keypoint_inputs, self.last_keypoint_inputs = False, None

    def _kp_modules(self):
        return (("roi_heads.keypoint_head.", self.keypoint_head), ("roi_heads.keypoint_predictor.", self.keypoint_predictor))

    def head_parameters(self):
        return super().head_parameters() + list(self.keypoint_head.parameters()) + list(self.keypoint_predictor.parameters())

    def state_dict(self, *a, **k):
        sd = super().state_dict(*a, **k)
        for pre, mod in self._kp_modules():
            for k2, v in mod.state_dict().items():
                sd[pre + k2] = v
        return sd

    def load_state_dict(self, sd, strict=True):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        super().load_state_dict(sd, strict)
        for pre, mod in self._kp_modules():
            sub = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
            if sub or strict:
                mod.load_state_dict(sub, strict=strict)

    # ------------------------------------------------------------------ the branch itself
    def _kp_forward(self, feats, rois, image_shapes):
        """rois [rows, 5] -> (pooled + the 8 head activations, sub-pixel logits fp32 [rows, 14, 14, 4 * KP], level tables)."""
        rows = rois.shape[0]
        lv = self.keypoint_roi_pool.levels_nhwc(feats, image_shapes)
        acts = [ops.mask_roi_pool(feats, rois, *lv)]
        for conv, pk in zip(self.keypoint_head.convs, self.keypoint_head._packs):
            wf, _wd, b = pk.get(conv.weight, conv.bias)
            y = torch.empty((rows, 14, 14, 512), device=rois.device, dtype=torch.bfloat16)
            ops.conv_fwd_ex(ops.conv_shape(rows, 14, 14, conv.in_channels, 512, 3, 1), acts[-1], wf, y, shift=b, relu=True)
            acts.append(y)
        pr = self.keypoint_predictor
        wf, _wd, b = pr._pack.get(pr.kps_score_lowres.weight, pr.kps_score_lowres.bias)
        z = torch.empty((rows, 14, 14, 4 * pr.kp), device=rois.device, dtype=torch.float32)
        ops.conv_fwd_ex(ops.conv_shape(rows, 14, 14, 512, 4 * pr.kp, 3, 1), acts[-1], wf, z, shift=b, out_f32=True)
        return acts, z, lv

    def _kp_backward(self, feats, rois, acts, z, lv, target, valid, count, num_rois):
        """keypointrcnn_loss + its gradients: parameter .grad accumulated, -> (loss_keypoint, fp32 NHWC feature gradients)."""
        rows = rois.shape[0]
        pr = self.keypoint_predictor
        dc = pr.kps_score_lowres
        loss, dz, dbias, *terms = ops.keypoint_loss(z, target, valid, count, want_terms=self.keep_keypoint_inputs)
        if terms and self.last_keypoint_inputs is not None:      # tests: every pair's loss term
            self.last_keypoint_inputs["loss_terms"] = terms[0][:num_rois]
        dshape = ops.conv_shape(rows, 14, 14, 512, 4 * pr.kp, 3, 1)
        _wf, wd, _b = pr._pack.get(dc.weight, dc.bias)
        dw = torch.zeros((4 * pr.kp, 9 * 512), device=z.device, dtype=torch.float32)
        ops.conv_wgrad(dshape, acts[-1], dz, dw)
        _acc_grad(dc.weight, subpixel_weight_grad(dw.reshape(4 * pr.kp, 3, 3, 512), 512, self.num_keypoints))
        _acc_grad(dc.bias, dbias)
        g = torch.empty((rows, 14, 14, 512), device=z.device, dtype=torch.bfloat16)
        ops.conv_dgrad_mask(dshape, dz, wd, g, acts[-1])
        convs, packs = self.keypoint_head.convs, self.keypoint_head._packs
        for i in range(len(convs) - 1, -1, -1):
            conv = convs[i]
            cin = conv.in_channels
            shape = ops.conv_shape(rows, 14, 14, cin, 512, 3, 1)
            _wf, wd, _b = packs[i].get(conv.weight, conv.bias)
            dw = torch.zeros((512, 9 * cin), device=z.device, dtype=torch.float32)
            db = torch.zeros(512, device=z.device, dtype=torch.float32)
            ops.conv_wgrad(shape, acts[i], g, dw, dbias=db)
            _acc_grad(conv.weight, dw.reshape(512, 3, 3, cin).permute(0, 3, 1, 2))
            _acc_grad(conv.bias, db)
            gi = torch.empty((rows, 14, 14, cin), device=z.device, dtype=torch.bfloat16)
            if i > 0:
                ops.conv_dgrad_mask(shape, g, wd, gi, acts[i])
            else:
                ops.conv_dgrad(shape, g, wd, gi)
            g = gi
        fgrads = ops.mask_roi_pool_bwd(feats, rois, *lv, g, num_rois=num_rois)
        return loss.reshape(()), fgrads

    def _zero_kp_grads(self):
        for p in list(self.keypoint_head.parameters()) + list(self.keypoint_predictor.parameters()):
            _acc_grad(p, torch.zeros_like(p))

    def _roi_extra_train(self, feats, proposals, matched_idxs, labels, targets, image_shapes, fused, losses):
        """roi_heads.py:894-922: positives (labels > 0) of the sampled RoIs and their matched gt -> loss_keypoint."""
        if any("keypoints" not in t for t in targets):
            raise ValueError("KeypointRCNN: targets[i]['keypoints'] is required in training")
        for t in targets:
            kp = t["keypoints"]
            if kp.dim() != 3 or kp.shape[1] != self.num_keypoints or kp.shape[2] != 3 or kp.shape[0] != t["boxes"].shape[0]:
                raise ValueError(f"KeypointRCNN: expected target keypoints of shape [G, {self.num_keypoints}, 3], got {tuple(kp.shape)}")
        dev = feats[0].device
        if fused:
            rois, mi, lab = proposals, matched_idxs, labels[0]
            r = int(sum(self.roi_targets.last_num_pos))
        else:
            rois = torch.cat([torch.cat([torch.full((p.shape[0], 1), i, dtype=p.dtype, device=dev), p], 1) for i, p in enumerate(proposals)])
            mi, lab = torch.cat(matched_idxs), torch.cat(labels)
            r = int((lab > 0).sum())
        self.last_keypoint_rows = r
        if r == 0:                              # roi_heads.py:351-352: keypoint_logits.sum() * 0
            losses["loss_keypoint"] = torch.zeros((), device=dev)
            self._zero_kp_grads()
            return None
        rows = _rows_for(r)
        pos = torch.nonzero_static(lab > 0, size=rows, fill_value=0).squeeze(1)
        krois, kgt = rois[pos].contiguous(), mi[pos].contiguous()
        target, valid, count = ops.keypoint_targets([t["keypoints"].to(dev) for t in targets], krois, kgt, 56, valid_rows=r)
        acts, z, lv = self._kp_forward(feats, krois, image_shapes)
        if self.keep_keypoint_inputs:      # tests: what the branch saw (RoIs, matched gt, pooled features, targets) for a CPU re-run
            self.last_keypoint_inputs = dict(rois=krois[:r].clone(), gt_index=kgt[:r].clone(), pooled=acts[0][:r].clone(),
                                             target=target[:r].clone(), valid=valid[:r].clone(), count=count.clone())
        loss, fgrads = self._kp_backward(feats, krois, acts, z, lv, target, valid, count, r)
        losses["loss_keypoint"] = loss
        return fgrads

    def _roi_extra_eval(self, feats, detections, image_shapes):
        """roi_heads.py:923-930: keypoints [D, K, 3] and keypoints_scores [D, K] of the detections, in the transformed image's frame."""
        dev = feats[0].device
        K = self.num_keypoints
        counts = [int(d["boxes"].shape[0]) for d in detections]
        total = sum(counts)
        if total == 0:
            for d in detections:
                d["keypoints"] = torch.zeros((0, K, 3), device=dev)
                d["keypoints_scores"] = torch.zeros((0, K), device=dev)
            return detections
        rows = _rows_for(total)
        rois = torch.zeros((rows, 5), device=dev, dtype=torch.float32)
        o = 0
        for i, (d, c) in enumerate(zip(detections, counts)):
            rois[o:o + c, 0] = i
            rois[o:o + c, 1:] = d["boxes"]
            o += c
        rois[total:] = rois[0]
        with torch.no_grad():
            _acts, z, _lv = self._kp_forward(feats, rois, image_shapes)
            maps = ops.keypoint_heatmaps(z[:total], K)
            if self.keep_keypoint_inputs:
                self.last_keypoint_inputs = dict(rois=rois[:total].clone(), maps=maps)
            xy, scores = ops.heatmaps_to_keypoints(maps, rois[:total])
        o = 0
        for d, c in zip(detections, counts):
            d["keypoints"] = xy[o:o + c]
            d["keypoints_scores"] = scores[o:o + c]
            o += c
        return detections


def keypointrcnn_resnet50_fpn(pretrained=False, progress=True, num_classes=2, num_keypoints=17, pretrained_backbone=False,
                              trainable_backbone_layers=None, tfidf=None, **kwargs):
    """torchvision's keypointrcnn_resnet50_fpn (signature from memory).  No network here: `pretrained*` must be False; load weights with
    `load_state_dict`."""
    if pretrained or pretrained_backbone:
        raise NotImplementedError("no network access: load a reference state_dict with model.load_state_dict(...)")
    if trainable_backbone_layers is None:
        trainable_backbone_layers = 3
    return KeypointRCNN(num_classes, trainable_backbone_layers, tfidf=tfidf, num_keypoints=num_keypoints, **kwargs)
