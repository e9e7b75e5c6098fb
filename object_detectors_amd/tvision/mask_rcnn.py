"""Mirror of the reference `MaskRCNN` / `maskrcnn_resnet50_fpn` (tvision/mask_rcnn.py:21-300) and the mask branch of `RoIHeads.forward`
(tvision/roi_heads.py:844-887) over the MI355X kernels.

    model = maskrcnn_resnet50_fpn(num_classes=91)
    losses = model(images, targets)     # + 'loss_mask'; targets[i]['masks'] = uint8 [G_i, H_i, W_i]; backward already done
    detections = model(images)          # eval: [{'boxes','labels','scores','masks'}], masks [D,1,H0,W0] (list input) or [D,1,28,28]
    MaskRCNN(mask_format="rle")         # eval on a list input: masks = RLEBatch, the COCO run lengths of `masks > 0.5` at H0 x W0, made
                                        # from the 28x28 probabilities by one fused kernel pair (mi355det_mask_rle_count / _emit)

Everything of Faster R-CNN (tvision/frcnn.py) is inherited unchanged; the mask branch runs as
  * mask_roi_pool   MultiScaleRoIAlign(['0'..'3'], 14, 2) into bf16 NHWC [R, 14, 14, 256] (mi355det_mask_roi_pool; backward: fp32 atomics);
  * mask_head       4 x Conv2d(256, 256, 3, pad 1) + ReLU: mi355det_conv_fwd_ex (bias + ReLU epilogue), mi355det_conv_dgrad_mask (the ReLU
                    backward of the layer below folded in), mi355det_conv_wgrad - the MFMA kernels of the backbone;
  * conv5_mask      ConvTranspose2d(256, 256, 2, stride=2) + ReLU as the 1x1 convolution 256 -> 1024 of the same kernels, output kept in
                    sub-pixel order [R, 14, 14, 4*256] (channel q*256 + co is mask pixel (2i + q // 2, 2j + q % 2)); its weight gradient
                    (no bias term: conv_wgrad's bias sum uses atomics) is fixed-order, its bias gradient comes out of mi355det_mask_loss;
  * mask_fcn_logits + maskrcnn_loss   one fused kernel on the label channel only (mi355det_mask_loss), never materialising [R, K, 28, 28];
  * project_masks_on_boxes            mi355det_mask_targets (all images, one launch);
  * maskrcnn_inference / paste        mi355det_mask_probs, mi355det_paste_masks (GeneralizedRCNNTransform.postprocess).

Row buckets: the number of positives R changes every step (at most box_batch_size_per_image * positive_fraction per image).  The mask branch
runs on rows = MASK_BUCKET * ceil(R / MASK_BUCKET) (at least one bucket); padded rows repeat RoI 0 and get zero loss gradient, so they add
nothing to any weight gradient and are skipped by the pooling backward.  The convolution tile choices are per shape and made without timing
outside a plan build, so a step with a new bucket runs no autotune.  The row count comes from the sampler's host counts: the branch adds no
host read to the Faster R-CNN step.
Parameters are ordinary fp32 torch parameters with the reference's names (state-dict keys roi_heads.mask_head.mask_fcn{1..4}.*,
roi_heads.mask_predictor.{conv5_mask,mask_fcn_logits}.*) and initialisation; gradients land in their .grad (head_parameters() lists them for
the torch optimizer / ParamGradSync); the bf16 packs are rebuilt when a parameter's version counter moves.
"""
from collections import OrderedDict

import torch
from torch import nn

from .. import ops
from .frcnn import FasterRCNN
from .roi_align import MultiScaleRoIAlign

MASK_BUCKET = 32


def _rows_for(r):
    return max(MASK_BUCKET, (r + MASK_BUCKET - 1) // MASK_BUCKET * MASK_BUCKET)


def _acc_grad(p, g):
    g = g.reshape(p.shape)
    if p.grad is None:
        p.grad = g.contiguous().clone()
    else:
        p.grad.add_(g)


class _Packed:
    """bf16 forward / data-gradient packs of one fp32 parameter pair, rebuilt when a version counter moves (tvision/linear.py)."""

    def __init__(self, master_fn, shape):
        self.master_fn, self.shape, self.key, self.val = master_fn, shape, None, None

    def get(self, weight, bias):
        key = (weight._version, weight.data_ptr(), bias._version, bias.data_ptr())
        if key != self.key:
            w, b = self.master_fn(weight.detach(), bias.detach())
            wf, wd = ops.pack_weights(self.shape, w.float().contiguous())
            self.val, self.key = (wf, wd, b.float().contiguous()), key
        return self.val


class MaskRCNNHeads(nn.Module):
    """mask_rcnn.py:226-248: mask_fcn{i} = Conv2d(3x3, padding=dilation) + ReLU.  The Conv2d modules hold the parameters (reference names and
    init); the computation is MaskRCNN._mask_forward / _mask_backward."""

    def __init__(self, in_channels, layers, dilation):
        super().__init__()
        if dilation != 1 or in_channels != 256 or any(l != 256 for l in layers):
            raise NotImplementedError("MaskRCNNHeads: the HIP path covers 256-channel layers with dilation 1 (the reference's default)")
        d = OrderedDict()
        nxt = in_channels
        for i, f in enumerate(layers, 1):
            d[f"mask_fcn{i}"] = nn.Conv2d(nxt, f, kernel_size=3, stride=1, padding=dilation, dilation=dilation)
            d[f"relu{i}"] = nn.ReLU(inplace=True)
            nxt = f
        for k, m in d.items():
            self.add_module(k, m)
        for name, param in self.named_parameters():
            if "weight" in name:
                nn.init.kaiming_normal_(param, mode="fan_out", nonlinearity="relu")
        self.convs = [d[f"mask_fcn{i}"] for i in range(1, len(layers) + 1)]
        shape = ops.conv_shape(MASK_BUCKET, 14, 14, 256, 256, 3, 1)
        self._packs = [_Packed(lambda w, b: (w, b), shape) for _ in self.convs]

    def forward(self, x):
        raise RuntimeError("MaskRCNNHeads runs inside MaskRCNN (HIP kernels); there is no eager forward")


class MaskRCNNPredictor(nn.Module):
    """mask_rcnn.py:251-264: conv5_mask = ConvTranspose2d(in, dim_reduced, 2, 2, 0) + ReLU, mask_fcn_logits = Conv2d(dim_reduced, K, 1)."""

    def __init__(self, in_channels, dim_reduced, num_classes):
        super().__init__()
        if in_channels != 256 or dim_reduced != 256:
            raise NotImplementedError("MaskRCNNPredictor: the HIP path covers in_channels = dim_reduced = 256 (the reference's default)")
        self.conv5_mask = nn.ConvTranspose2d(in_channels, dim_reduced, 2, 2, 0)
        self.relu = nn.ReLU(inplace=True)
        self.mask_fcn_logits = nn.Conv2d(dim_reduced, num_classes, 1, 1, 0)
        for name, param in self.named_parameters():
            if "weight" in name:
                nn.init.kaiming_normal_(param, mode="fan_out", nonlinearity="relu")
        # [in, out, 2, 2] -> 1x1 convolution [q*256 + co, ci], q = 2*di + dj; the bias repeats per sub-pixel
        shape = ops.conv_shape(MASK_BUCKET, 14, 14, 256, 1024, 1, 1)
        self._pack = _Packed(lambda w, b: (w.permute(2, 3, 1, 0).reshape(1024, 256, 1, 1), b.repeat(4)), shape)

    def forward(self, x):
        raise RuntimeError("MaskRCNNPredictor runs inside MaskRCNN (HIP kernels); there is no eager forward")


class MaskRCNN(FasterRCNN):
    """mask_rcnn.py:21-223 over tvision/frcnn.py:FasterRCNN (same constructor arguments, the box classifier's long-tail baselines
    loss_type='seesaw' | 'eql' with eql_tail= among them)."""

    def __init__(self, num_classes=91, trainable_backbone_layers=3, tfidf=None, mask_roi_pool=None, mask_head=None, mask_predictor=None,
                 mask_format="dense", **kw):
        super().__init__(num_classes, trainable_backbone_layers, tfidf=tfidf, **kw)
        if mask_format not in ("dense", "rle"):
            raise ValueError("MaskRCNN: mask_format must be 'dense' or 'rle'")
        self.mask_format = mask_format
        dev = self.engine.device
        if mask_roi_pool is not None and (not isinstance(mask_roi_pool, MultiScaleRoIAlign) or mask_roi_pool.output_size != (14, 14)):
            raise NotImplementedError("MaskRCNN: mask_roi_pool must be a 14x14 MultiScaleRoIAlign")
        self.mask_roi_pool = mask_roi_pool or MultiScaleRoIAlign(["0", "1", "2", "3"], 14, 2)
        self.mask_head = (mask_head or MaskRCNNHeads(256, (256, 256, 256, 256), 1)).to(dev)
        self.mask_predictor = (mask_predictor or MaskRCNNPredictor(256, 256, num_classes)).to(dev)
        self.last_mask_rows = None
        self.keep_mask_inputs, self.last_mask_inputs = False, None

    @property
    def _postprocess_kw(self):
        return {} if self.mask_format == "dense" else {"mask_format": self.mask_format}

    def head_parameters(self):
        return super().head_parameters() + list(self.mask_head.parameters()) + list(self.mask_predictor.parameters())

    def state_dict(self, *a, **k):
        sd = super().state_dict(*a, **k)
        for k2, v in self.mask_head.state_dict().items():
            sd["roi_heads.mask_head." + k2] = v
        for k2, v in self.mask_predictor.state_dict().items():
            sd["roi_heads.mask_predictor." + k2] = v
        return sd

    def load_state_dict(self, sd, strict=True):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        super().load_state_dict(sd, strict)
        for pre, mod in (("roi_heads.mask_head.", self.mask_head), ("roi_heads.mask_predictor.", self.mask_predictor)):
            sub = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
            if sub or strict:
                mod.load_state_dict(sub, strict=strict)

    # ------------------------------------------------------------------ the branch itself
    def _mask_forward(self, feats, rois, image_shapes):
        """rois [rows, 5] -> (pooled + the 4 head activations, deconvolution output [rows, 14, 14, 1024] bf16, level tables)."""
        rows = rois.shape[0]
        lv = self.mask_roi_pool.levels_nhwc(feats, image_shapes)
        x = ops.mask_roi_pool(feats, rois, *lv)
        acts = [x]
        shape = ops.conv_shape(rows, 14, 14, 256, 256, 3, 1)
        for conv, pk in zip(self.mask_head.convs, self.mask_head._packs):
            wf, _wd, b = pk.get(conv.weight, conv.bias)
            y = torch.empty((rows, 14, 14, 256), device=rois.device, dtype=torch.bfloat16)
            ops.conv_fwd_ex(shape, acts[-1], wf, y, shift=b, relu=True)
            acts.append(y)
        dc = self.mask_predictor.conv5_mask
        wf, _wd, b = self.mask_predictor._pack.get(dc.weight, dc.bias)
        z = torch.empty((rows, 14, 14, 1024), device=rois.device, dtype=torch.bfloat16)
        ops.conv_fwd_ex(ops.conv_shape(rows, 14, 14, 256, 1024, 1, 1), acts[-1], wf, z, shift=b, relu=True)
        return acts, z, lv

    def _mask_backward(self, feats, rois, acts, z, lv, labels, mask_targets, valid):
        """maskrcnn_loss + its gradients: parameter .grad accumulated, -> (loss_mask, fp32 NHWC feature gradients)."""
        rows = rois.shape[0]
        pr = self.mask_predictor
        lg = pr.mask_fcn_logits
        loss, dz, dwl, dbl, dbd = ops.mask_loss(z, lg.weight.detach().reshape(lg.weight.shape[0], 256), lg.bias.detach(), labels, mask_targets, valid)
        _acc_grad(lg.weight, dwl)
        _acc_grad(lg.bias, dbl)
        dshape = ops.conv_shape(rows, 14, 14, 256, 1024, 1, 1)
        _wf, wd, _b = pr._pack.get(pr.conv5_mask.weight, pr.conv5_mask.bias)
        dw = torch.zeros((1024, 256), device=z.device, dtype=torch.float32)
        ops.conv_wgrad(dshape, acts[-1], dz, dw)
        _acc_grad(pr.conv5_mask.weight, dw.reshape(2, 2, 256, 256).permute(3, 2, 0, 1))
        _acc_grad(pr.conv5_mask.bias, dbd)
        g = torch.empty((rows, 14, 14, 256), device=z.device, dtype=torch.bfloat16)
        ops.conv_dgrad_mask(dshape, dz, wd, g, acts[-1])
        shape = ops.conv_shape(rows, 14, 14, 256, 256, 3, 1)
        for i in range(len(self.mask_head.convs) - 1, -1, -1):
            conv, pk = self.mask_head.convs[i], self.mask_head._packs[i]
            _wf, wd, _b = pk.get(conv.weight, conv.bias)
            dw = torch.zeros((256, 9 * 256), device=z.device, dtype=torch.float32)
            db = torch.zeros(256, device=z.device, dtype=torch.float32)
            ops.conv_wgrad(shape, acts[i], g, dw, dbias=db)
            _acc_grad(conv.weight, dw.reshape(256, 3, 3, 256).permute(0, 3, 1, 2))
            _acc_grad(conv.bias, db)
            gi = torch.empty_like(g)
            if i > 0:
                ops.conv_dgrad_mask(shape, g, wd, gi, acts[i])
            else:
                ops.conv_dgrad(shape, g, wd, gi)
            g = gi
        fgrads = ops.mask_roi_pool_bwd(feats, rois, *lv, g, num_rois=valid)
        return loss.reshape(()), fgrads

    def _zero_mask_grads(self):
        for p in list(self.mask_head.parameters()) + list(self.mask_predictor.parameters()):
            _acc_grad(p, torch.zeros_like(p))

    def _roi_extra_train(self, feats, proposals, matched_idxs, labels, targets, image_shapes, fused, losses):
        """roi_heads.py:844-875: positives (labels > 0) of the sampled RoIs and their matched gt -> loss_mask."""
        if any("masks" not in t for t in targets):
            raise ValueError("MaskRCNN: targets[i]['masks'] is required in training")
        dev = feats[0].device
        if fused:
            rois, mi, lab = proposals, matched_idxs, labels[0]
            r = int(sum(self.roi_targets.last_num_pos))
        else:
            rois = torch.cat([torch.cat([torch.full((p.shape[0], 1), i, dtype=p.dtype, device=dev), p], 1) for i, p in enumerate(proposals)])
            mi, lab = torch.cat(matched_idxs), torch.cat(labels)
            r = int((lab > 0).sum())
        self.last_mask_rows = r
        if r == 0:                              # roi_heads.py:175-178: mask_logits.sum() * 0
            losses["loss_mask"] = torch.zeros((), device=dev)
            self._zero_mask_grads()
            return None
        rows = _rows_for(r)
        pos = torch.nonzero_static(lab > 0, size=rows, fill_value=0).squeeze(1)
        mrois, mgt, mlab = rois[pos].contiguous(), mi[pos].contiguous(), lab[pos].contiguous()
        tgt = ops.mask_targets([t["masks"] for t in targets], mrois, mgt, 28, num_rois=r)
        acts, z, lv = self._mask_forward(feats, mrois, image_shapes)
        if self.keep_mask_inputs:           # tests: what the branch saw (RoIs, matched gt, labels, pooled features) for a CPU re-run
            self.last_mask_inputs = dict(rois=mrois[:r].clone(), gt_index=mgt[:r].clone(), labels=mlab[:r].clone(), pooled=acts[0][:r].clone())
        loss, fgrads = self._mask_backward(feats, mrois, acts, z, lv, mlab, tgt, r)
        losses["loss_mask"] = loss
        return fgrads

    def _roi_extra_eval(self, feats, detections, image_shapes):
        """roi_heads.py:876-883: masks of the detections = sigmoid of the predicted label's channel, [D, 1, 28, 28] per image."""
        dev = feats[0].device
        counts = [int(d["boxes"].shape[0]) for d in detections]
        total = sum(counts)
        if total == 0:
            for d in detections:
                d["masks"] = torch.zeros((0, 1, 28, 28), device=dev)
            return detections
        rows = _rows_for(total)
        rois = torch.zeros((rows, 5), device=dev, dtype=torch.float32)
        labels = torch.zeros(rows, device=dev, dtype=torch.int64)
        o = 0
        for i, (d, c) in enumerate(zip(detections, counts)):
            rois[o:o + c, 0] = i
            rois[o:o + c, 1:] = d["boxes"]
            labels[o:o + c] = d["labels"]
            o += c
        rois[total:] = rois[0]
        with torch.no_grad():
            _acts, z, _lv = self._mask_forward(feats, rois, image_shapes)
            lg = self.mask_predictor.mask_fcn_logits
            probs = ops.mask_probs(z, lg.weight.detach().reshape(lg.weight.shape[0], 256), lg.bias.detach(), labels)
        o = 0
        for d, c in zip(detections, counts):
            d["masks"] = probs[o:o + c, None]
            o += c
        return detections


def maskrcnn_resnet50_fpn(pretrained=False, progress=True, num_classes=91, pretrained_backbone=False, trainable_backbone_layers=None, tfidf=None,
                          **kwargs):
    """mask_rcnn.py:272-334.  No network here: `pretrained*` must be False; load weights with `load_state_dict`."""
    if pretrained or pretrained_backbone:
        raise NotImplementedError("no network access: load a reference state_dict with model.load_state_dict(...)")
    if trainable_backbone_layers is None:
        trainable_backbone_layers = 3
    return MaskRCNN(num_classes, trainable_backbone_layers, tfidf=tfidf, **kwargs)
