"""Tensor-level wrappers over the C ABI (include/mi355det.h).

PyTorch is plumbing here: it owns device memory and the stream; every computation below runs
in libmi355det.so.  All tensors must live on the GPU; nothing falls back to torch ops.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import HeadView, YoloGeom, YoloLossCfg, check, ptr, stream_ptr

# ---- storage format seen by the convolution helpers below: "bf16" (default) or, inside `with ops.storage("fp16"):`, the fp16 twins of the
#      entry points (include/mi355det_f16.h) and torch.float16 buffers.  The engines carry their own format (YoloV3Engine(storage=...)).
_STORAGE = ["bf16"]


def lib():
    return _lib.storage_lib(_STORAGE[0])


def act_dtype():
    return torch.float16 if _STORAGE[0] == "fp16" else torch.bfloat16


class storage:
    def __init__(self, fmt):
        if fmt not in ("bf16", "fp16"):
            raise ValueError("storage must be 'bf16' or 'fp16'")
        self.fmt = fmt

    def __enter__(self):
        self.prev = _STORAGE[0]
        _STORAGE[0] = self.fmt
        return self

    def __exit__(self, *exc):
        _STORAGE[0] = self.prev
        return False



def _f32c(t):
    if not t.is_cuda:
        raise ValueError("mi355det ops need CUDA/HIP tensors (no CPU fallback)")
    return t.contiguous().float()


# ----------------------------------------------------------------------------------------- YOLO
def make_geom(anchors, num_classes, img_size, grids, iou_type=1, ignore_thr=0.5):
    """anchors: per scale list of (w,h) pixels, scale order = head order (stride 32,16,8).
    Normalised anchor sizes are computed exactly like yolo_forw.py:99,108-113 (float64 divide,
    float32 store, float32 divide by grid)."""
    import numpy as np
    g = YoloGeom()
    ns, na = len(grids), len(anchors[0])
    if ns > _lib.MAX_SCALES or na > _lib.MAX_ANCHORS:
        raise ValueError("unsupported number of scales / anchors per scale")
    g.num_scales, g.na, g.num_classes = ns, na, num_classes
    g.img_size, g.ignore_thr, g.iou_type = float(img_size), float(ignore_thr), int(iou_type)
    off = 0
    for k, gr in enumerate(grids):
        g.grid[k] = int(gr)
        g.off[k] = off
        off += gr * gr * na
        stride = img_size / gr
        for a, (aw, ah) in enumerate(anchors[k]):
            g.anchor_w[k][a] = float(np.float32(np.float32(aw / stride) / np.float32(gr)))
            g.anchor_h[k][a] = float(np.float32(np.float32(ah / stride) / np.float32(gr)))
    for k in range(ns, _lib.MAX_SCALES + 1):
        g.off[k] = off
    return g


def head_views(heads, attrs_total, dtype=torch.float32):
    """NCHW-shaped tensors [bs, A*attrs, H, W] with any (dense-pixel) strides -> HeadView array."""
    arr = (HeadView * _lib.MAX_SCALES)()
    keep = []
    for k, t in enumerate(heads):
        if t.dim() != 4 or t.shape[1] != attrs_total:
            raise ValueError(f"head {k}: expected [bs,{attrs_total},H,W], got {tuple(t.shape)}")
        if t.dtype != dtype or t.stride(2) != t.shape[3] * t.stride(3):
            if dtype != torch.float32:
                raise ValueError("gradient views must already be bf16 with dense pixel strides")
            t = t.float().contiguous()
        keep.append(t)
        arr[k].ptr = t.data_ptr()
        arr[k].sb, arr[k].sc, arr[k].sp = t.stride(0), t.stride(1), t.stride(3)
    return arr, keep


def flatten_targets(targets, device):
    """list of {'bbox': [M,4], 'category_id': [M]} -> (boxes [G,4] f32, labels [G] i64, off [bs+1] i32, counts)."""
    counts = [int(t["bbox"].shape[0]) for t in targets]
    boxes = torch.cat([t["bbox"].reshape(-1, 4) for t in targets]).to(device=device, dtype=torch.float32).contiguous()
    labels = torch.cat([t["category_id"].reshape(-1) for t in targets]).to(device=device, dtype=torch.int64).contiguous()
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    off = torch.tensor(offs, dtype=torch.int32).to(device, non_blocking=True)
    return boxes, labels, off, counts


def bbox_iou(bb1, bb2, iou_type, xcycwh=True):
    """helper.bbox_iou: broadcast [M,1,4]x[1,N,4] -> [M,N], or same-shape [n,4] -> [n]."""
    bb1, bb2 = _f32c(bb1), _f32c(bb2)
    if bb1.dim() == 3 and bb2.dim() == 3 and bb1.shape[1] == 1 and bb2.shape[0] == 1:
        m, n = bb1.shape[0], bb2.shape[1]
        out = torch.empty((m, n), device=bb1.device, dtype=torch.float32)
        check(lib().mi355det_bbox_iou(ptr(bb1), ptr(bb2), ptr(out), m, n, int(iou_type), int(xcycwh), 0, stream_ptr()), "bbox_iou")
        return out
    if bb1.shape != bb2.shape or bb1.shape[-1] != 4:
        raise ValueError("bbox_iou: shapes must be [M,1,4]x[1,N,4] or equal [...,4]")
    n = bb1.numel() // 4
    out = torch.empty(bb1.shape[:-1], device=bb1.device, dtype=torch.float32)
    check(lib().mi355det_bbox_iou(ptr(bb1), ptr(bb2), ptr(out), 1, n, int(iou_type), int(xcycwh), 1, stream_ptr()), "bbox_iou")
    return out


def yolo_assign(geom, boxes, off, bs, counts):
    """YOLOForw.get_target for the whole batch -> (obj_idx [G] i64, tgt [G,4], noobj [bs,N] u8)."""
    dev = boxes.device
    G, N = boxes.shape[0], geom.off[geom.num_scales]
    key = torch.empty(max(G, 1), device=dev, dtype=torch.int64)
    obj_idx = torch.empty(G, device=dev, dtype=torch.int64)
    tgt = torch.empty((G, 4), device=dev, dtype=torch.float32)
    noobj = torch.empty((bs, N), device=dev, dtype=torch.uint8)
    check(lib().mi355det_yolo_assign(C.byref(geom), ptr(boxes), ptr(off), bs, G, max(counts) if counts else 0, ptr(key),
                                     ptr(obj_idx), ptr(tgt), ptr(noobj), stream_ptr()), "yolo_assign")
    return obj_idx, tgt, noobj


def yolo_loss(geom, cfg, hviews, gviews, off, labels, obj_idx, tgt, noobj, idf, bs, G):
    dev = labels.device
    N = geom.off[geom.num_scales]
    wsb = lib().mi355det_yolo_loss_workspace(bs, N)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    out12 = torch.empty(12, device=dev, dtype=torch.float32)
    check(lib().mi355det_yolo_loss(C.byref(geom), C.byref(cfg), hviews, gviews, ptr(off), ptr(labels), ptr(obj_idx), ptr(tgt),
                                   ptr(noobj), ptr(idf), bs, G, ptr(ws), wsb, ptr(out12), stream_ptr()), "yolo_loss")
    return out12


def yolo_decode(geom, hviews, idf, bs, softmax_cls=True, want_scores=False):
    """-> decoded [bs,N,attrs] (and, with want_scores on channels-last heads, score [bs,N] + arg-max label [bs,N])."""
    N, attrs = geom.off[geom.num_scales], geom.num_classes + 5
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((bs, N, attrs), device=dev, dtype=torch.float32)
    score = label = None
    if want_scores and all(hviews[k].sc == 1 for k in range(geom.num_scales)):
        score = torch.empty((bs, N), device=dev, dtype=torch.float32)
        label = torch.empty((bs, N), device=dev, dtype=torch.int32)
    check(lib().mi355det_yolo_decode(C.byref(geom), hviews, ptr(idf), bs, int(softmax_cls), ptr(out), ptr(score), ptr(label), stream_ptr()),
          "yolo_decode")
    return (out, score, label) if want_scores else out


def yolo_candidates(pred, conf_thr, max_cand=None, score=None, label=None):
    """test_one_epoch.py:24-35 -> (cand [bs,max_cand,6], count [bs] i32).  score/label: the fused outputs of yolo_decode."""
    pred = _f32c(pred)
    bs, n, attrs = pred.shape
    max_cand = int(max_cand or min(n, 16384))
    cand = torch.empty((bs, max_cand, 6), device=pred.device, dtype=torch.float32)
    count = torch.empty(bs, device=pred.device, dtype=torch.int32)
    wsb = lib().mi355det_yolo_candidates_workspace(bs, n)
    ws = torch.empty(wsb, device=pred.device, dtype=torch.uint8)
    check(lib().mi355det_yolo_candidates(ptr(pred), ptr(score), ptr(label), bs, n, attrs, float(conf_thr), ptr(cand), ptr(count), max_cand,
                                         ptr(ws), wsb, stream_ptr()), "yolo_candidates")
    return cand, count


def nms_majority_batched(boxes, count, thresh_iou, num_classes):
    """boxes [bs,max_n,6], count [bs] i32 -> (rows [bs,max_n,6], idx [bs,max_n] i32, kept [bs] i32)."""
    boxes = _f32c(boxes)
    bs, max_n, _ = boxes.shape
    rows = torch.empty_like(boxes)
    idx = torch.empty((bs, max_n), device=boxes.device, dtype=torch.int32)
    kept = torch.empty(bs, device=boxes.device, dtype=torch.int32)
    wsb = lib().mi355det_nms_workspace(bs, max_n)
    ws = torch.empty(wsb, device=boxes.device, dtype=torch.uint8)
    check(lib().mi355det_nms_majority(ptr(boxes), ptr(count), bs, max_n, float(thresh_iou), int(num_classes), ptr(rows), ptr(idx),
                                      ptr(kept), ptr(ws), wsb, stream_ptr()), "nms_majority")
    return rows, idx, kept


# ------------------------------------------------------------------------------- torchvision side
def box_iou(boxes1, boxes2):
    b1, b2 = _f32c(boxes1), _f32c(boxes2)
    out = torch.empty((b1.shape[0], b2.shape[0]), device=b1.device, dtype=torch.float32)
    check(lib().mi355det_box_iou(ptr(b1), ptr(b2), ptr(out), b1.shape[0], b2.shape[0], stream_ptr()), "box_iou")
    return out


def nms_raw(boxes, scores, iou_threshold, idxs=None):
    """nms / batched_nms without the host round trip: (keep [n] int64 - only the first `count` entries are defined -, count [1] int32 on
    the device).  Callers that post-process several images read all their counts with ONE transfer."""
    boxes, scores = _f32c(boxes), _f32c(scores)
    n = boxes.shape[0]
    if idxs is not None:
        idxs = idxs.to(torch.int64).contiguous()
    keep = torch.zeros(max(n, 1), device=boxes.device, dtype=torch.int64)
    cnt = torch.zeros(1, device=boxes.device, dtype=torch.int32)
    if n:
        wsb = lib().mi355det_nms_workspace(1, n)
        ws = torch.empty(wsb, device=boxes.device, dtype=torch.uint8)
        check(lib().mi355det_nms(ptr(boxes), ptr(scores), ptr(idxs), n, float(iou_threshold), ptr(keep), ptr(cnt), ptr(ws), wsb,
                                 stream_ptr()), "nms")
    return keep, cnt


def nms_batch(boxes, scores, iou_threshold, idxs=None):
    """`bs` independent NMS problems of the same size in one launch sequence: boxes [bs,n,4], scores [bs,n], idxs [bs,n] (categories, as
    batched_nms) or None -> (keep [bs,n] int64 - the first counts[b] entries of row b are defined -, counts [bs] int32 on the device)."""
    boxes, scores = _f32c(boxes), _f32c(scores)
    bs, n = scores.shape
    if idxs is not None:
        idxs = idxs.to(torch.int64).contiguous()
    keep = torch.zeros((bs, max(n, 1)), device=boxes.device, dtype=torch.int64)
    cnt = torch.zeros(bs, device=boxes.device, dtype=torch.int32)
    if n and bs:
        wsb = lib().mi355det_nms_workspace(bs, n)
        ws = torch.empty(wsb, device=boxes.device, dtype=torch.uint8)
        check(lib().mi355det_nms_batch(ptr(boxes), ptr(scores), ptr(idxs), bs, n, float(iou_threshold), ptr(keep), ptr(cnt), ptr(ws), wsb,
                                       stream_ptr()), "nms_batch")
    return keep, cnt


def rpn_proposals(objectness, deltas, anchors, clip_limits, level_counts, pre_nms_top_n, post_nms_top_n, nms_thresh, score_thresh=0.0,
                  min_size=1e-3, xform_clip=math.log(1000.0 / 16), counts_out=None):
    """RegionProposalNetwork.filter_proposals (rpn.py:215-280) incl. the decode of the selected anchors, whole batch, one host call:
    objectness [N,A] logits, deltas [N,A,4], anchors [A,4], clip_limits [N,4] = (w,h,w,h) -> (boxes [N,post,4], scores [N,post],
    counts [N] int32 on the device; rows beyond counts[i] are zero)."""
    objectness, deltas, anchors, clip_limits = _f32c(objectness), _f32c(deltas), _f32c(anchors), _f32c(clip_limits)
    n, a = objectness.shape
    if deltas.numel() != n * a * 4 or anchors.numel() != a * 4 or clip_limits.numel() != n * 4 or sum(level_counts) != a:
        raise ValueError("rpn_proposals: objectness [N,A], deltas [N,A,4], anchors [A,4], clip_limits [N,4], sum(level_counts) == A")
    lc = (C.c_int64 * len(level_counts))(*[int(v) for v in level_counts])
    wsb = lib().mi355det_rpn_proposals_workspace(n, lc, len(level_counts), int(pre_nms_top_n))
    if wsb == 0:
        raise ValueError("rpn_proposals: need 1..8 non-empty levels, a positive batch and pre_nms_top_n")
    dev = objectness.device
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    boxes = torch.empty((n, int(post_nms_top_n), 4), device=dev, dtype=torch.float32)
    scores = torch.empty((n, int(post_nms_top_n)), device=dev, dtype=torch.float32)
    counts = counts_out if counts_out is not None else torch.empty(n, device=dev, dtype=torch.int32)
    check(lib().mi355det_rpn_proposals(ptr(objectness), ptr(deltas), ptr(anchors), ptr(clip_limits), n, lc, len(level_counts), int(pre_nms_top_n),
                                       int(post_nms_top_n), float(nms_thresh), float(score_thresh), float(min_size), float(xform_clip),
                                       ptr(boxes), ptr(scores), ptr(counts), ptr(ws), wsb, stream_ptr()), "rpn_proposals")
    return boxes, scores, counts


def retina_detections(cls_logits_per_level, bbox_reg_per_level, anchors_per_level, clip_limits, logit_thresh, topk_candidates, nms_thresh,
                      detections_per_img, xform_clip=math.log(1000.0 / 16)):
    """RetinaNet.postprocess_detections (retinanet.py:414-472), whole batch, one host call: per level cls_logits [N,HWA,K] (fp32, tf-idf
    scaling already applied), bbox regression [N,HWA,4], anchors [HWA,4]; clip_limits [N,4] = (w,h,w,h) ->
    (boxes [N,det,4], scores [N,det], labels [N,det] i64, counts [N] i32 on the device)."""
    cl = [_f32c(t) for t in cls_logits_per_level]
    rg = [_f32c(t) for t in bbox_reg_per_level]
    an = [_f32c(t) for t in anchors_per_level]
    clip_limits = _f32c(clip_limits)
    nl, n, k = len(cl), cl[0].shape[0], cl[0].shape[-1]
    hwa = [int(t.shape[1]) for t in cl]
    if not 1 <= nl <= 8 or any(r.shape[:2] != c.shape[:2] or a.shape[0] != c.shape[1] for c, r, a in zip(cl, rg, an)) or clip_limits.numel() != 4 * n:
        raise ValueError("retina_detections: 1..8 levels of cls_logits [N,HWA,K], bbox_regression [N,HWA,4], anchors [HWA,4]; clip_limits [N,4]")
    i64a, vpa = C.c_int64 * nl, C.c_void_p * nl
    la = i64a(*hwa)
    wsb = lib().mi355det_retina_detections_workspace(n, la, nl, k, int(topk_candidates))
    if wsb == 0:
        raise ValueError("retina_detections: need fewer than 2^32 scores per image and level and 1 <= topk_candidates <= 16384")
    dev = cl[0].device
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    det = int(detections_per_img)
    boxes = torch.empty((n, det, 4), device=dev, dtype=torch.float32)
    scores = torch.empty((n, det), device=dev, dtype=torch.float32)
    labels = torch.empty((n, det), device=dev, dtype=torch.int64)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    check(lib().mi355det_retina_detections(vpa(*[ptr(t) for t in cl]), vpa(*[ptr(t) for t in rg]), vpa(*[ptr(t) for t in an]), la, nl, n, k,
                                           ptr(clip_limits), float(logit_thresh), int(topk_candidates), float(nms_thresh), det, float(xform_clip),
                                           ptr(boxes), ptr(scores), ptr(labels), ptr(counts), ptr(ws), wsb, stream_ptr()), "retina_detections")
    return boxes, scores, labels, counts


def roi_detections(scores, box_regression, proposals, clip_limits, score_thresh, max_candidates, weights, nms_thresh, detections_per_img,
                   min_size=1e-2, xform_clip=math.log(1000.0 / 16), meta_out=None):
    """RoIHeads.postprocess_detections (roi_heads.py:715-781), whole batch, one host call: scores [N,P,C] (class 0 / padded proposals already
    below the threshold), box_regression [N,P,C*4], proposals [N,P,4], clip_limits [N,4] -> (boxes [N,det,4], scores [N,det], labels [N,det],
    meta [2N] i32 = detections per image, then candidates per image (== max_candidates: possibly truncated))."""
    scores, box_regression, proposals, clip_limits = _f32c(scores), _f32c(box_regression), _f32c(proposals), _f32c(clip_limits)
    n, p, c = scores.shape
    k = int(min(max_candidates, p * c))
    if box_regression.numel() != n * p * c * 4 or proposals.numel() != n * p * 4 or clip_limits.numel() != n * 4:
        raise ValueError("roi_detections: scores [N,P,C], box_regression [N,P,C*4], proposals [N,P,4], clip_limits [N,4]")
    wsb = lib().mi355det_roi_detections_workspace(n, p, c, k)
    if wsb == 0:
        raise ValueError("roi_detections: need 1 <= max_candidates <= 16384 and fewer than 2^32 scores per image")
    dev = scores.device
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    det = int(detections_per_img)
    boxes = torch.empty((n, det, 4), device=dev, dtype=torch.float32)
    out_s = torch.empty((n, det), device=dev, dtype=torch.float32)
    labels = torch.empty((n, det), device=dev, dtype=torch.int64)
    meta = meta_out if meta_out is not None else torch.empty(2 * n, device=dev, dtype=torch.int32)
    check(lib().mi355det_roi_detections(ptr(scores), ptr(box_regression), ptr(proposals), ptr(clip_limits), n, p, c, float(score_thresh), k,
                                        *[float(w) for w in weights], float(xform_clip), float(min_size), float(nms_thresh), det, ptr(boxes),
                                        ptr(out_s), ptr(labels), ptr(meta[:n]), ptr(meta[n:]), ptr(ws), wsb, stream_ptr()), "roi_detections")
    return boxes, out_s, labels, meta, k


def rpn_loss(objectness, pred_bbox_deltas, labels, regression_targets, pos_idx, sampled_idx):
    """RegionProposalNetwork.compute_loss (rpn.py:282-318) with its gradients, one launch: objectness [T(,1)], deltas / targets [T,4],
    labels [T] float, pos_idx / sampled_idx int64 -> (losses [2] = (objectness, box), grad_objectness like objectness, grad_deltas [T,4])."""
    obj, dl, lab, tg = _f32c(objectness), _f32c(pred_bbox_deltas), _f32c(labels), _f32c(regression_targets)
    t = obj.numel()
    if dl.numel() != 4 * t or lab.numel() != t or tg.numel() != 4 * t or sampled_idx.numel() == 0:
        raise ValueError("rpn_loss: objectness [T], deltas / targets [T,4], labels [T], at least one sampled anchor")
    pos_idx, sampled_idx = pos_idx.to(torch.int64).contiguous(), sampled_idx.to(torch.int64).contiguous()
    losses = torch.empty(2, device=obj.device, dtype=torch.float32)
    g_obj, g_dl = torch.empty_like(obj), torch.empty_like(dl)
    check(lib().mi355det_rpn_loss(ptr(obj), ptr(dl), ptr(lab), ptr(tg), t, ptr(pos_idx) if pos_idx.numel() else None, pos_idx.numel(),
                                  ptr(sampled_idx), sampled_idx.numel(), ptr(losses), ptr(g_obj), ptr(g_dl), stream_ptr()), "rpn_loss")
    return losses, g_obj, g_dl


def roi_match(proposals, proposal_counts, gt_boxes, gt_labels, gt_offsets, fg_iou_thresh, bg_iou_thresh, counts_out=None):
    """RoIHeads.assign_targets_to_proposals over add_gt_proposals (roi_heads.py:627-652,664-668) for the whole batch, one launch: proposals
    [N,P,4] padded + proposal_counts [N] i32 on the device, gt_boxes [G,4] / gt_labels [G] concatenated, gt_offsets host list [N+1] ->
    (matched [N,C] i32, labels [N,C] i32, counts [N,2] i32 = positives / negatives), C = P + the largest ground-truth count."""
    proposals, gt_boxes = _f32c(proposals), _f32c(gt_boxes)
    n, p = proposals.shape[0], proposals.shape[1]
    if len(gt_offsets) != n + 1 or any(b <= a for a, b in zip(gt_offsets, gt_offsets[1:])):
        raise ValueError("No ground-truth boxes available for one of the images during training")          # Matcher, _utils.py:282-291
    c = p + max(b - a for a, b in zip(gt_offsets, gt_offsets[1:]))
    dev = proposals.device
    matched = torch.empty((n, c), device=dev, dtype=torch.int32)
    labels = torch.empty((n, c), device=dev, dtype=torch.int32)
    counts = counts_out if counts_out is not None else torch.empty((n, 2), device=dev, dtype=torch.int32)
    offs = (C.c_int32 * (n + 1))(*[int(v) for v in gt_offsets])
    check(lib().mi355det_roi_match(ptr(proposals), ptr(proposal_counts), n, p, ptr(gt_boxes), ptr(gt_labels.to(torch.int64).contiguous()), offs,
                                   float(fg_iou_thresh), float(bg_iou_thresh), c, ptr(matched), ptr(labels), ptr(counts), stream_ptr()), "roi_match")
    return matched, labels, counts


def roi_sample(proposals, proposal_counts, gt_boxes, gt_offsets, matched, labels, perm_pos, perm_neg, num_pos, num_neg, weights):
    """BalancedPositiveNegativeSampler's selection from its `randperm` draws + the gathers and BoxCoder.encode of select_training_samples
    (roi_heads.py:654-713), whole batch, one launch -> (rois [S,5], labels [S] i64, matched [S] i64, regression_targets [S,4])."""
    n, p = proposals.shape[0], proposals.shape[1]
    total = int(sum(num_pos) + sum(num_neg))
    dev = proposals.device
    rois = torch.empty((total, 5), device=dev, dtype=torch.float32)
    out_l = torch.empty(total, device=dev, dtype=torch.int64)
    out_m = torch.empty(total, device=dev, dtype=torch.int64)
    reg = torch.empty((total, 4), device=dev, dtype=torch.float32)
    vpa, i32a = C.c_void_p * n, C.c_int32 * n
    offs = (C.c_int32 * (n + 1))(*[int(v) for v in gt_offsets])
    check(lib().mi355det_roi_sample(ptr(proposals), ptr(proposal_counts), n, p, ptr(gt_boxes), offs, matched.shape[1], ptr(matched), ptr(labels),
                                    vpa(*[ptr(t) for t in perm_pos]), vpa(*[ptr(t) for t in perm_neg]), i32a(*[int(v) for v in num_pos]),
                                    i32a(*[int(v) for v in num_neg]), *[float(w) for w in weights], ptr(rois), ptr(out_l), ptr(out_m), ptr(reg),
                                    stream_ptr()), "roi_sample")
    return rois, out_l, out_m, reg


def nms(boxes, scores, iou_threshold, idxs=None):
    boxes, scores = _f32c(boxes), _f32c(scores)
    n = boxes.shape[0]
    if n == 0:
        return torch.empty(0, device=boxes.device, dtype=torch.int64)
    if idxs is not None:
        idxs = idxs.to(torch.int64).contiguous()
    keep = torch.empty(n, device=boxes.device, dtype=torch.int64)
    cnt = torch.empty(1, device=boxes.device, dtype=torch.int32)
    wsb = lib().mi355det_nms_workspace(1, n)
    ws = torch.empty(wsb, device=boxes.device, dtype=torch.uint8)
    check(lib().mi355det_nms(ptr(boxes), ptr(scores), ptr(idxs), n, float(iou_threshold), ptr(keep), ptr(cnt), ptr(ws), wsb,
                             stream_ptr()), "nms")
    return keep[: int(cnt.item())]


def match_anchors(gt, anchors, high, low, allow_low_quality):
    gt, anchors = _f32c(gt), _f32c(anchors)
    m, n = gt.shape[0], anchors.shape[0]
    if m == 0:
        raise ValueError("No ground-truth boxes available for one of the images during training")
    if n == 0:
        raise ValueError("No proposal boxes available for one of the images during training")
    best = torch.empty(m, device=gt.device, dtype=torch.int32)
    out = torch.empty(n, device=gt.device, dtype=torch.int64)
    check(lib().mi355det_match_anchors(ptr(gt), ptr(anchors), m, n, float(high), float(low), int(allow_low_quality), ptr(best),
                                       ptr(out), stream_ptr()), "match_anchors")
    return out


def box_encode(reference_boxes, proposals, weights):
    r, p = _f32c(reference_boxes), _f32c(proposals)
    out = torch.empty_like(p)
    check(lib().mi355det_box_encode(ptr(r), ptr(p), ptr(out), p.shape[0], *[float(w) for w in weights], stream_ptr()), "box_encode")
    return out


def box_decode(rel_codes, boxes, weights, clip):
    c, b = _f32c(rel_codes), _f32c(boxes)
    n, k = b.shape[0], c.shape[1] // 4
    out = torch.empty_like(c)
    check(lib().mi355det_box_decode(ptr(c), ptr(b), ptr(out), n, k, *[float(w) for w in weights], float(clip), stream_ptr()),
          "box_decode")
    return out


def anchor_grid(cell, gh, gw, sh, sw):
    cell = _f32c(cell)
    out = torch.empty((gh * gw * cell.shape[0], 4), device=cell.device, dtype=torch.float32)
    check(lib().mi355det_anchor_grid(ptr(cell), cell.shape[0], gh, gw, int(sh), int(sw), ptr(out), stream_ptr()), "anchor_grid")
    return out


def sigmoid_focal_loss_sum(x, t, alpha, gamma, scale=None, valid=None, want_grad=True, grad_scale=1.0):
    """sum-reduced loss and its gradient wrt x in one pass: x,t [rows,k]."""
    x, t = _f32c(x), _f32c(t)
    rows, k = (x.shape[0], x.shape[1]) if x.dim() == 2 else (x.numel(), 1)
    loss = torch.zeros(1, device=x.device, dtype=torch.float32)
    grad = torch.empty_like(x) if want_grad else None
    if valid is not None:
        valid = valid.to(torch.uint8).contiguous()
    check(lib().mi355det_sigmoid_focal_loss(ptr(x), ptr(t), ptr(scale), ptr(valid), rows, k, float(alpha), float(gamma),
                                            float(grad_scale), ptr(loss), ptr(grad), stream_ptr()), "sigmoid_focal_loss")
    return loss[0], grad


def sigmoid_focal_loss_elem(x, t, alpha, gamma, want_grad=True):
    """Unreduced focal loss (reduction='none') and its derivative, elementwise on any shape."""
    x, t = _f32c(x), _f32c(t)
    if x.shape != t.shape:
        raise ValueError("inputs and targets must have the same shape")
    loss = torch.empty_like(x)
    grad = torch.empty_like(x) if want_grad else None
    check(lib().mi355det_sigmoid_focal_loss_elem(ptr(x), ptr(t), x.numel(), float(alpha), float(gamma), ptr(loss), ptr(grad), stream_ptr()),
          "sigmoid_focal_loss_elem")
    return loss, grad


def retina_cls_loss_sum(logits, matched, gt_labels, alpha, gamma, scale=None, want_grad=True, grad_scale=1.0):
    logits = _f32c(logits)
    rows, k = logits.shape
    loss = torch.zeros(1, device=logits.device, dtype=torch.float32)
    grad = torch.empty_like(logits) if want_grad else None
    check(lib().mi355det_retina_cls_loss(ptr(logits), ptr(matched.contiguous()), ptr(gt_labels.to(torch.int64).contiguous()),
                                         ptr(scale), rows, k, float(alpha), float(gamma), float(grad_scale), ptr(loss), ptr(grad),
                                         stream_ptr()), "retina_cls_loss")
    return loss[0], grad


# ------------------------------------------------------------------------------------ conv path
def conv_shape(n, h, w, cin, cout, ksize, stride, in_ld=None, out_ld=None):
    pad = (ksize - 1) // 2
    ho, wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    return _lib.ConvShape(n, h, w, cin, ho, wo, cout, ksize, stride, pad, in_ld or cin, out_ld or cout)


def pad_to(v, m):
    return (v + m - 1) // m * m


def cout_pad_of(cout):
    if cout >= 2048:
        return pad_to(cout, 256)        # very wide outputs (the 1204-class RetinaNet head: 10 836): whole 256-channel tiles for igemm8
    return pad_to(cout, 128) if cout >= 128 or cout % 32 else cout


def pack_weights(shape, w_master, want_dgrad=True, ohwi=False, wf=None, wd=None):
    """fp32 [cout,cin,k,k] (or OHWI [cout,k,k,cin]) -> (bf16 fwd pack [cout_pad, k*k*cin], bf16 dgrad pack)."""
    dev = w_master.device
    cp = cout_pad_of(shape.cout)
    kk = shape.ksize * shape.ksize
    if wf is None:
        wf = torch.empty(cp * kk * shape.cin, device=dev, dtype=act_dtype())
    if want_dgrad and wd is None:
        wd = torch.empty(lib().mi355det_dgrad_pack_elems(C.byref(shape)), device=dev, dtype=act_dtype())
    check(lib().mi355det_pack_weights(C.byref(shape), ptr(w_master.contiguous()), int(ohwi), ptr(wf), cp, ptr(wd), stream_ptr()),
          "pack_weights")
    return wf, wd


def conv_fwd(shape, x, w_fwd, y, bias=None, out_f32=False, stats=None):
    cp = cout_pad_of(shape.cout)
    check(lib().mi355det_conv_fwd(C.byref(shape), ptr(x), ptr(w_fwd), ptr(bias), ptr(y), int(out_f32), ptr(stats), cp, stream_ptr()),
          "conv_fwd")


def conv_stats_rows(shape):
    return lib().mi355det_conv_stats_rows(C.byref(shape), cout_pad_of(shape.cout))


def conv_dgrad(shape, dy, w_dgrad, dx, residual=None, residual_ld=0):
    check(lib().mi355det_conv_dgrad(C.byref(shape), ptr(dy), ptr(w_dgrad), ptr(dx), ptr(residual), int(residual_ld), stream_ptr()),
          "conv_dgrad")


def conv_dgrad_mask(shape, dy, w_dgrad, dx, act, act_ld=None, scale=None, relu=True):
    """dx = bf16(conv2d_input(dy)) * scale * (act > 0): the data gradient with the ReLU (/ frozen affine) backward of the layer that produced
    the convolution's input folded in (stride 1)."""
    check(lib().mi355det_conv_dgrad_mask(C.byref(shape), ptr(dy), ptr(w_dgrad), ptr(dx), ptr(act), int(act_ld or shape.in_ld), ptr(scale),
                                         int(bool(relu)), stream_ptr()), "conv_dgrad_mask")


_WGRAD_WS = {}


def conv_wgrad(shape, x, dy, dw, dbias=None, workspace=None):
    need = lib().mi355det_conv_wgrad_workspace(C.byref(shape))
    if workspace is None and need:
        key = dw.device
        if key not in _WGRAD_WS or _WGRAD_WS[key].numel() < need:
            _WGRAD_WS[key] = torch.empty(need, device=dw.device, dtype=torch.uint8)
        workspace = _WGRAD_WS[key]
    check(lib().mi355det_conv_wgrad(C.byref(shape), ptr(x), ptr(dy), ptr(dw), ptr(dbias), ptr(workspace),
                                    workspace.numel() if workspace is not None else 0, stream_ptr()), "conv_wgrad")


# ------------------------------------------------------------------------------------ grouped 3x3 convolution (bf16 storage only)
def gconv_shape(n, h, w, c, stride=1, in_ld=None, out_ld=None):
    """ConvShape of a grouped 3x3 convolution: c = cin = cout are the totals (the group count is a separate argument of every call)."""
    return conv_shape(n, h, w, c, c, 3, stride, in_ld, out_ld)


def gconv_pack(shape, groups, w_master, ohwi=False, want_dgrad=True, wf=None, wd=None):
    """fp32 [cout, cin/groups, 3, 3] (or OHWI [cout, 3, 3, cin/groups]) -> (forward image, data-gradient image), both bf16."""
    elems = _lib.lib().mi355det_gconv_pack_elems(C.byref(shape), groups)
    if not elems:
        check(-1, "gconv_pack")
    if wf is None:
        wf = torch.empty(elems, device=w_master.device, dtype=torch.bfloat16)
    if want_dgrad and wd is None:
        wd = torch.empty(elems, device=w_master.device, dtype=torch.bfloat16)
    check(_lib.lib().mi355det_gconv_pack_weights(C.byref(shape), groups, ptr(_f32c(w_master)), int(ohwi), ptr(wf), ptr(wd) if want_dgrad else None,
                                                 stream_ptr()), "gconv_pack_weights")
    return wf, (wd if want_dgrad else None)


def gconv_fwd(shape, groups, x, w_fwd, y, scale=None, shift=None, relu=False):
    e = _lib.ConvEpilogue(ptr(scale), ptr(shift), None, 0, int(bool(relu)), 0)
    check(_lib.lib().mi355det_gconv_fwd_ex(C.byref(shape), groups, ptr(x), ptr(w_fwd), C.byref(e), ptr(y), 0, stream_ptr()), "gconv_fwd_ex")


def gconv_dgrad(shape, groups, dy, w_dgrad, dx):
    check(_lib.lib().mi355det_gconv_dgrad(C.byref(shape), groups, ptr(dy), ptr(w_dgrad), ptr(dx), stream_ptr()), "gconv_dgrad")


def gconv_wgrad(shape, groups, x, dy, dw, workspace=None):
    """dw fp32 [cout, 3, 3, cin/groups] is written (not accumulated); fixed summation order."""
    need = _lib.lib().mi355det_gconv_wgrad_workspace(C.byref(shape), groups)
    if workspace is None:
        workspace = torch.empty(max(need, 16), device=dw.device, dtype=torch.uint8)
    check(_lib.lib().mi355det_gconv_wgrad(C.byref(shape), groups, ptr(x), ptr(dy), ptr(dw), ptr(workspace), workspace.numel(), stream_ptr()),
          "gconv_wgrad")


# ------------------------------------------------------------------------------------ RoIAlign / top-k
def roi_align_multi(feats, rois, output_size, scales, sampling_ratio=2, aligned=False, k_min=2, k_max=5, grad_out=None):
    """feats: list of NCHW fp32 maps (1..4 levels); rois [K,5].  Forward -> [K,C,ph,pw]; with grad_out -> list of dfeats."""
    feats = [_f32c(f) for f in feats]
    rois = _f32c(rois)
    nl = len(feats)
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    K, Cc = rois.shape[0], feats[0].shape[1]
    P = (C.c_void_p * nl)(*[f.data_ptr() for f in feats])
    hs = (C.c_int32 * nl)(*[f.shape[2] for f in feats])
    ws = (C.c_int32 * nl)(*[f.shape[3] for f in feats])
    sc = (C.c_float * nl)(*[float(s) for s in scales])
    if grad_out is None:
        out = torch.empty((K, Cc, ph, pw), device=rois.device, dtype=torch.float32)
        check(lib().mi355det_roi_align(P, hs, ws, sc, nl, ptr(rois), K, Cc, ph, pw, int(sampling_ratio), int(aligned), k_min, k_max,
                                       ptr(out), None, None, stream_ptr()), "roi_align")
        return out
    g = _f32c(grad_out)
    dfs = [torch.zeros_like(f) for f in feats]
    G = (C.c_void_p * nl)(*[d.data_ptr() for d in dfs])
    check(lib().mi355det_roi_align(P, hs, ws, sc, nl, ptr(rois), K, Cc, ph, pw, int(sampling_ratio), int(aligned), k_min, k_max,
                                   None, ptr(g), G, stream_ptr()), "roi_align_bwd")
    return dfs


def topk_rows(x, k, min_value=float("-inf")):
    """x [rows,n] fp32 -> (values [rows,k], indices [rows,k] i64, count [rows] i32), descending, ties lower index first."""
    x = _f32c(x)
    rows, n = x.shape
    k = int(min(k, n))
    idx = torch.zeros((rows, k), device=x.device, dtype=torch.int64)
    val = torch.zeros((rows, k), device=x.device, dtype=torch.float32)
    cnt = torch.empty(rows, device=x.device, dtype=torch.int32)
    if n >= 65536:          # long rows (flattened HWA x K score maps): several workgroups per row
        wsb = lib().mi355det_topk_workspace(rows)
        ws = torch.empty(wsb, device=x.device, dtype=torch.uint8)
        check(lib().mi355det_topk_ws(ptr(x), rows, n, x.stride(0), k, float(min_value), ptr(idx), ptr(val), ptr(cnt), ptr(ws), wsb, stream_ptr()), "topk")
        return val, idx, cnt
    check(lib().mi355det_topk(ptr(x), rows, n, x.stride(0), k, float(min_value), ptr(idx), ptr(val), ptr(cnt), stream_ptr()), "topk")
    return val, idx, cnt


def topk_segments(x, seg_counts, k, min_value=float("-inf")):
    """x [rows, sum(seg_counts)] fp32: top-min(k, n_s) of every segment of every row in one call (RegionProposalNetwork._get_top_n_idx,
    rpn.py:215-228) -> list per segment of (values [rows,k_s], indices within the segment [rows,k_s] i64, count [rows] i32)."""
    x = _f32c(x)
    rows, a = x.shape
    if sum(seg_counts) != a or not 1 <= len(seg_counts) <= 8:
        raise ValueError("topk_segments: 1..8 segments that add up to the row length")
    ns = len(seg_counts)
    ks = [int(min(k, n)) for n in seg_counts]
    starts = [sum(seg_counts[:i]) for i in range(ns)]
    outs = [(torch.zeros((rows, kk), device=x.device, dtype=torch.float32), torch.zeros((rows, kk), device=x.device, dtype=torch.int64),
             torch.empty(rows, device=x.device, dtype=torch.int32)) for kk in ks]
    wsb = lib().mi355det_topk_workspace(rows)
    ws = torch.empty(wsb, device=x.device, dtype=torch.uint8)
    i64a, i32a, vpa = C.c_int64 * ns, C.c_int32 * ns, C.c_void_p * ns
    check(lib().mi355det_topk_segments(ptr(x), rows, x.stride(0), ns, i64a(*starts), i64a(*[int(n) for n in seg_counts]), i32a(*ks), float(min_value),
                                       vpa(*[ptr(o[1]) for o in outs]), vpa(*[ptr(o[0]) for o in outs]), vpa(*[ptr(o[2]) for o in outs]),
                                       ptr(ws), wsb, stream_ptr()), "topk_segments")
    return outs


# ------------------------------------------------------------------------------------ ResNet-FPN / RetinaNet companions
def conv_fwd_ex(shape, x, w_fwd, y, scale=None, shift=None, residual=None, residual_ld=0, relu=False, out_f32=False, out_image_stride=0,
                leaky_slope=None):
    """y = relu?(conv(x,w)*scale + shift + residual): FrozenBatchNorm2d / bias / identity add fused into the conv epilogue.
    leaky_slope: Darknet form y = lrelu(conv*scale + shift) + residual."""
    mode = 2 if leaky_slope is not None else int(bool(relu))
    e = _lib.ConvEpilogue(ptr(scale), ptr(shift), ptr(residual), int(residual_ld), mode, int(out_image_stride), float(leaky_slope or 0.0))
    check(lib().mi355det_conv_fwd_ex(C.byref(shape), ptr(x), ptr(w_fwd), C.byref(e), ptr(y), int(out_f32), cout_pad_of(shape.cout), stream_ptr()),
          "conv_fwd_ex")


def im2col_nchw(img, ksize, stride, pad, kpad, mean=None, inv_std=None):
    n, c, h, w = img.shape
    ho, wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    out = torch.empty((n, ho, wo, kpad), device=img.device, dtype=torch.bfloat16)
    check(lib().mi355det_im2col_nchw(ptr(_f32c(img)), ptr(mean), ptr(inv_std), ptr(out), n, c, h, w, ksize, stride, pad, kpad, stream_ptr()),
          "im2col_nchw")
    return out


def maxpool3x3s2(x):
    n, h, w, c = x.shape
    out = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), device=x.device, dtype=torch.bfloat16)
    check(lib().mi355det_maxpool3x3s2(ptr(x), c, n, h, w, c, ptr(out), c, stream_ptr()), "maxpool3x3s2")
    return out


def relu_affine_bwd(g1, a, scale=None, g2=None, relu=True, want_gm=False):
    c = g1.shape[-1]
    pixels = g1.numel() // c
    dz = torch.empty_like(g1)
    gm = torch.empty_like(g1) if want_gm else None
    check(lib().mi355det_relu_affine_bwd(ptr(g1), c, ptr(g2), c if g2 is not None else 0, ptr(a), c, ptr(scale), c, pixels, int(relu), ptr(dz), c,
                                         ptr(gm), c, stream_ptr()), "relu_affine_bwd")
    return (dz, gm) if want_gm else dz


def upsample_nearest_add(x, lateral, out_hw):
    n, h, w, c = x.shape
    out = torch.empty((n, out_hw[0], out_hw[1], c), device=x.device, dtype=torch.bfloat16)
    check(lib().mi355det_upsample_nearest_add(ptr(x), c, n, h, w, c, ptr(lateral), c if lateral is not None else 0, out_hw[0], out_hw[1], ptr(out), c,
                                              stream_ptr()), "upsample_nearest_add")
    return out


def upsample_nearest_bwd(g, hw, accumulate=None):
    n, gh, gw, c = g.shape
    out = torch.empty((n, hw[0], hw[1], c), device=g.device, dtype=torch.bfloat16)
    check(lib().mi355det_upsample_nearest_bwd(ptr(g), c, n, hw[0], hw[1], c, gh, gw, ptr(accumulate), c if accumulate is not None else 0, ptr(out), c,
                                              stream_ptr()), "upsample_nearest_bwd")
    return out


def retina_loss(cls_logits, bbox_regression, anchors, matched, gt_boxes, gt_labels, gt_offsets, k=None, class_scale=None, alpha=0.25, gamma=2.0,
                want_grad=True, grad_scale=1.0, grad_logits=None, grad_regression=None, cls_levels=None, anchors_per_pixel=None):
    """Batched RetinaNetHead.compute_loss.  -> (losses[2] = (classification, bbox_regression), num_fg [N], grad_logits, grad_regression).
    cls_levels (list of bf16 [n, h, w, ld] buffers, one per pyramid level, + anchors_per_pixel): the class gradient is written there in the
    head convolution's layout instead of an fp32 grad_logits (returned as None)."""
    n, rows, k = cls_logits.shape
    dev = cls_logits.device
    losses = torch.empty(2, device=dev)
    nfg = torch.empty(n, device=dev)
    if cls_levels is not None:
        from ._lib import LevelGrads
        if len(cls_levels) > 8 or not anchors_per_pixel:
            raise ValueError("retina_loss: at most 8 levels, and anchors_per_pixel is required with cls_levels")
        lv = LevelGrads()
        lv.n_levels, lv.anchors_per_pixel = len(cls_levels), int(anchors_per_pixel)
        for q, t in enumerate(cls_levels):
            if t.dtype != torch.bfloat16 or t.dim() != 4 or t.shape[0] != n or not t.is_contiguous():
                raise ValueError("retina_loss: cls_levels must be contiguous bf16 [n, h, w, ld] tensors")
            lv.pixels[q], lv.grad[q], lv.grad_ld[q] = t.shape[1] * t.shape[2], t.data_ptr(), t.shape[3]
        grad_regression = torch.empty_like(bbox_regression) if grad_regression is None else grad_regression
        check(lib().mi355det_retina_loss_lv(ptr(cls_logits), ptr(bbox_regression), ptr(anchors), ptr(matched), ptr(gt_boxes), ptr(gt_labels),
                                            ptr(gt_offsets), ptr(class_scale), n, rows, k, float(alpha), float(gamma), float(grad_scale), ptr(nfg),
                                            ptr(losses), C.byref(lv), ptr(grad_regression), stream_ptr()), "retina_loss_lv")
        return losses, nfg, None, grad_regression
    if want_grad:
        grad_logits = torch.empty_like(cls_logits) if grad_logits is None else grad_logits
        grad_regression = torch.empty_like(bbox_regression) if grad_regression is None else grad_regression
    check(lib().mi355det_retina_loss(ptr(cls_logits), ptr(bbox_regression), ptr(anchors), ptr(matched), ptr(gt_boxes), ptr(gt_labels), ptr(gt_offsets),
                                     ptr(class_scale), n, rows, k, float(alpha), float(gamma), float(grad_scale), ptr(nfg), ptr(losses),
                                     ptr(grad_logits) if want_grad else None, ptr(grad_regression) if want_grad else None, stream_ptr()), "retina_loss")
    return losses, nfg, grad_logits, grad_regression


def conv_dgrad_bn(shape, dy, w_dgrad, dx, z, scale_shift, slope, residual=None, residual_ld=0):
    """dgrad + fused BN-backward partial sums of the layer that produced dx's activation -> sums [2*cin]."""
    L = lib()
    rows = L.mi355det_conv_dgrad_bn_rows(C.byref(shape))
    cin_pad = pad_to(shape.cin, 32)
    partials = torch.empty((rows + 64, 2, cin_pad), device=dx.device, dtype=torch.float32)
    check(L.mi355det_conv_dgrad_bn(C.byref(shape), ptr(dy), ptr(w_dgrad), ptr(dx), ptr(residual), int(residual_ld), ptr(z), shape.in_ld,
                                   ptr(scale_shift), float(slope), ptr(partials), stream_ptr()), "conv_dgrad_bn")
    sums = torch.empty(2 * shape.cin, device=dx.device, dtype=torch.float32)
    check(L.mi355det_bn_bwd_sum_partials(ptr(partials), rows, shape.cin, cin_pad, ptr(sums), stream_ptr()), "bn_bwd_sum_partials")
    return sums


def _level_tables(feats, scales):
    """ctypes tables (pointers, heights, widths, pixel pitches, scales) of 1..4 bf16 NHWC pyramid levels."""
    nl = len(feats)
    for f in feats:
        if f.dtype != torch.bfloat16 or f.dim() != 4 or f.stride(3) != 1:
            raise ValueError("channels-last RoIAlign expects bf16 [n,h,w,C] tensors with contiguous channels")
    return (nl, (C.c_void_p * nl)(*[f.data_ptr() for f in feats]), (C.c_int32 * nl)(*[f.shape[1] for f in feats]),
            (C.c_int32 * nl)(*[f.shape[2] for f in feats]), (C.c_int32 * nl)(*[f.stride(2) for f in feats]),
            (C.c_float * nl)(*[float(s) for s in scales]))


def roi_align_nhwc(feats, rois, output_size, scales, sampling_ratio=2, aligned=False, k_min=2, k_max=5, grad_out=None):
    """Channels-last RoIAlign: feats = list of bf16 NHWC maps [n,h,w,C] (1..4 levels, pixel pitch = stride(2)); rois [K,5].
    Forward -> fp32 [K,C,ph,pw]; with grad_out -> list of fp32 NHWC feature gradients."""
    nl, P, hs, ws, lds, sc = _level_tables(feats, scales)
    rois = _f32c(rois)
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    K, Cc = rois.shape[0], feats[0].shape[3]
    if grad_out is None:
        out = torch.empty((K, Cc, ph, pw), device=rois.device, dtype=torch.float32)
        check(lib().mi355det_roi_align_nhwc(P, hs, ws, lds, sc, nl, ptr(rois), K, Cc, ph, pw, int(sampling_ratio), int(aligned), k_min, k_max,
                                            ptr(out), None, None, stream_ptr()), "roi_align_nhwc")
        return out
    g = _f32c(grad_out)
    dfs = [torch.zeros((f.shape[0], f.shape[1], f.shape[2], Cc), device=f.device, dtype=torch.float32) for f in feats]
    G = (C.c_void_p * nl)(*[d.data_ptr() for d in dfs])
    check(lib().mi355det_roi_align_nhwc(P, hs, ws, lds, sc, nl, ptr(rois), K, Cc, ph, pw, int(sampling_ratio), int(aligned), k_min, k_max,
                                        None, ptr(g), G, stream_ptr()), "roi_align_nhwc_bwd")
    return dfs


FRCNN_LOSS_TYPES = {"ce": 0, "bce": 1, "focal_loss": 2, "gombit": 3, "gombit_fl": 4}


def fastrcnn_loss(class_logits, box_regression, labels, regression_targets, class_scale=None, class_weights=None, loss_type="ce", want_grad=True):
    """roi_heads.py:24-96 (+ the tf-idf scaling of its call site :826-827) -> (losses [2], grad_logits, grad_box)."""
    if loss_type not in FRCNN_LOSS_TYPES:
        raise ValueError(f"fastrcnn_loss: unknown loss_type {loss_type!r} (reference: 'ce', 'bce', 'focal_loss', 'gombit', 'gombit_fl')")
    x, b = _f32c(class_logits), _f32c(box_regression)
    n, k = x.shape
    if b.shape != (n, 4 * k):
        raise ValueError("fastrcnn_loss: box_regression must be [n, 4*k]")
    lab = labels.to(torch.int64).contiguous()
    tgt = _f32c(regression_targets)
    cs = None if class_scale is None else _f32c(class_scale.reshape(-1))
    cw = None if class_weights is None else _f32c(class_weights.reshape(-1))
    L = lib()
    wsb = L.mi355det_fastrcnn_loss_workspace(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    losses = torch.empty(2, dtype=torch.float32, device=x.device)
    gl = torch.empty_like(x) if want_grad else None
    gb = torch.empty_like(b) if want_grad else None
    check(L.mi355det_fastrcnn_loss(ptr(x), ptr(b), ptr(lab), ptr(tgt), ptr(cs), ptr(cw), n, k, FRCNN_LOSS_TYPES[loss_type], ptr(losses), ptr(gl),
                                   ptr(gb), ptr(ws), wsb, stream_ptr()), "fastrcnn_loss")
    return losses, gl, gb


# ---- long-tail baselines beside the five reference losses (csrc/longtail_kernels.hip)
FRCNN_LONGTAIL_TYPES = {"seesaw": 0, "eql": 1}


def label_histogram(labels, counts):
    """counts[labels[i]] += 1 in place: counts [k] int64 on the device, integer atomics (exact, run-to-run identical).  A label outside
    [0, k) is skipped.  -> counts."""
    if not (labels.is_cuda and counts.is_cuda):
        raise ValueError("mi355det ops need CUDA/HIP tensors (no CPU fallback)")
    if counts.dtype != torch.int64 or counts.dim() != 1 or not counts.is_contiguous():
        raise ValueError("label_histogram: counts must be a contiguous int64 vector")
    lab = labels.to(torch.int64).contiguous().reshape(-1)
    check(lib().mi355det_label_histogram(ptr(lab), lab.numel(), counts.numel(), ptr(counts), stream_ptr()), "label_histogram")
    return counts


def fastrcnn_loss_longtail(class_logits, box_regression, labels, regression_targets, loss_type, class_scale=None, counts=None, tail=None,
                           p=0.8, q=2.0, eps=1e-2, update_counts=True, want_grad=True):
    """Seesaw ('seesaw': counts [k] int64, updated in place with this call's labels before the loss reads it unless update_counts=False)
    or Equalization loss v1 ('eql': tail [k] of 0/1, tail[0] == 0) with the box loss of fastrcnn_loss -> (losses [2], grad_logits, grad_box).
    The rules: include/mi355det.h, "Long-tail baselines"."""
    if loss_type not in FRCNN_LONGTAIL_TYPES:
        raise ValueError(f"fastrcnn_loss_longtail: unknown loss_type {loss_type!r} ('seesaw' or 'eql')")
    x, b = _f32c(class_logits), _f32c(box_regression)
    n, k = x.shape
    if b.shape != (n, 4 * k):
        raise ValueError("fastrcnn_loss_longtail: box_regression must be [n, 4*k]")
    lab = labels.to(torch.int64).contiguous()
    tgt = _f32c(regression_targets)
    cs = None if class_scale is None else _f32c(class_scale.reshape(-1))
    if not lab.is_cuda or lab.shape != (n,) or tgt.shape != (n, 4) or (cs is not None and cs.shape != (k,)):
        raise ValueError("fastrcnn_loss_longtail: labels [n] and regression_targets [n, 4] on the device, class_scale [k]")
    if loss_type == "seesaw":
        if counts is None or not counts.is_cuda or counts.dtype != torch.int64 or counts.shape != (k,) or not counts.is_contiguous():
            raise ValueError("fastrcnn_loss_longtail: 'seesaw' needs counts, a contiguous int64 [k] tensor on the device")
        tail = None
    else:
        if tail is None or not tail.is_cuda or tail.shape != (k,):
            raise ValueError("fastrcnn_loss_longtail: 'eql' needs tail, a [k] tensor of 0/1 on the device")
        if getattr(tail, "_mi355det_tail_checked", None) != tail._version:      # the read synchronises: once per tensor and content, not
            if bool(tail[0] != 0):                                              # once per training step
                raise ValueError("fastrcnn_loss_longtail: tail[0] must be 0 (the background is no tail category)")
            tail._mi355det_tail_checked = tail._version
        if tail.dtype != torch.uint8 or not tail.is_contiguous():
            tail = (tail != 0).to(torch.uint8).contiguous()
        counts = None
    L = lib()
    wsb = L.mi355det_fastrcnn_loss_longtail_workspace(n, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    losses = torch.empty(2, dtype=torch.float32, device=x.device)
    gl = torch.empty_like(x) if want_grad else None
    gb = torch.empty_like(b) if want_grad else None
    check(L.mi355det_fastrcnn_loss_longtail(ptr(x), ptr(b), ptr(lab), ptr(tgt), ptr(cs), n, k, FRCNN_LONGTAIL_TYPES[loss_type], ptr(counts),
                                            ptr(tail), float(p), float(q), float(eps), int(bool(update_counts)), ptr(losses), ptr(gl), ptr(gb),
                                            ptr(ws), wsb, stream_ptr()), "fastrcnn_loss_longtail")
    return losses, gl, gb


def repeat_factors(image_index, category_index, img_freq, n_images, t=1e-3):
    """Repeat-factor sampling (Gupta et al., LVIS 2019): int32 device vectors [A] of (image, category) index pairs and img_freq [n_categories]
    int32 (category_frequencies' second result) -> r [n_images] float64, r_i = max over image i's annotations of max(1, sqrt(t / f_c)),
    f_c = img_freq[c] / n_images; 1 for an image without annotations.  Raises ValueError for an index outside its range."""
    for v in (image_index, category_index, img_freq):
        if not (torch.is_tensor(v) and v.is_cuda):
            raise ValueError("mi355det ops need CUDA/HIP tensors (no CPU fallback)")
        if v.dtype != torch.int32 or v.dim() != 1:
            raise ValueError("repeat_factors: int32 vectors expected")
    if image_index.shape != category_index.shape:
        raise ValueError("repeat_factors: one category index per image index")
    im, cat, df = image_index.contiguous(), category_index.contiguous(), img_freq.contiguous()
    n_images = int(n_images)
    r = torch.ones(max(n_images, 0), dtype=torch.float64, device=im.device)
    errors = torch.empty(1, dtype=torch.int32, device=im.device)
    with torch.cuda.device(im.device):
        check(lib().mi355det_repeat_factors(ptr(im), ptr(cat), int(im.shape[0]), ptr(df), n_images, int(df.shape[0]), float(t), ptr(r), ptr(errors),
                                            stream_ptr()), "repeat_factors")
    bad = int(errors.item())
    if bad:
        raise ValueError(f"repeat_factors: {bad} annotation(s) with an image index outside [0, {n_images}) or a category index outside "
                         f"[0, {int(df.shape[0])})")
    return r


# ------------------------------------------------------------------------------------ Mask R-CNN mask branch (csrc/mask_kernels.hip; the pooling: csrc/roi_kernels.hip)
def mask_roi_pool(feats, rois, scales, k_min, k_max, output_size=14, sampling_ratio=2, out=None):
    """MultiScaleRoIAlign(['0'..'3'], 14, 2) into bf16 NHWC [K, 14, 14, C] (mask_fcn1's input); == bf16(roi_align_nhwc) bit for bit."""
    rois = _f32c(rois)
    nl, P, hs, ws, lds, sc = _level_tables(feats, scales)
    K, Cc = rois.shape[0], feats[0].shape[3]
    if out is None:
        out = torch.empty((K, output_size, output_size, Cc), device=rois.device, dtype=torch.bfloat16)
    check(lib().mi355det_mask_roi_pool(P, hs, ws, lds, sc, nl, ptr(rois), K, Cc, output_size, output_size, int(sampling_ratio), k_min, k_max,
                                       ptr(out), out.stride(2), None, 0, None, stream_ptr()), "mask_roi_pool")
    return out


def mask_roi_pool_bwd(feats, rois, scales, k_min, k_max, grad, num_rois=None, sampling_ratio=2, grad_feats=None):
    """Backward of mask_roi_pool: grad bf16 NHWC [K, ph, pw, C] (rows >= num_rois are skipped) -> fp32 NHWC feature gradients (fp32 atomics;
    accumulated into grad_feats when given)."""
    rois = _f32c(rois)
    nl, P, hs, ws, lds, sc = _level_tables(feats, scales)
    K = rois.shape[0] if num_rois is None else int(num_rois)
    Cc = feats[0].shape[3]
    if grad.dtype != torch.bfloat16 or grad.stride(3) != 1:
        raise ValueError("mask_roi_pool_bwd: grad must be bf16 NHWC with contiguous channels")
    if grad_feats is None:
        grad_feats = [torch.zeros((f.shape[0], f.shape[1], f.shape[2], Cc), device=f.device, dtype=torch.float32) for f in feats]
    G = (C.c_void_p * nl)(*[d.data_ptr() for d in grad_feats])
    check(lib().mi355det_mask_roi_pool(P, hs, ws, lds, sc, nl, ptr(rois), K, Cc, grad.shape[1], grad.shape[2], int(sampling_ratio), k_min, k_max,
                                       None, 0, ptr(grad), grad.stride(2), G, stream_ptr()), "mask_roi_pool_bwd")
    return grad_feats


def mask_targets(masks, rois, gt_index, m=28, num_rois=None):
    """project_masks_on_boxes for a whole batch in one launch: masks = per-image uint8 [G_b, h_b, w_b]; rois [R,5] = (image, box);
    gt_index [R] int64 = matched gt inside the image -> fp32 [R, m, m] (rows >= num_rois are left unwritten)."""
    rois = _f32c(rois)
    if len(masks) > _lib.MASK_MAX_IMAGES:
        raise ValueError(f"mask_targets: at most {_lib.MASK_MAX_IMAGES} images")
    imgs = _lib.MaskImages()
    keep = []
    for b, mk in enumerate(masks):
        mk = mk.to(torch.uint8).contiguous()
        if mk.dim() != 3 or not mk.is_cuda:
            raise ValueError("mask_targets: masks must be CUDA uint8 [G, h, w] per image")
        keep.append(mk)
        imgs.masks[b], imgs.h[b], imgs.w[b] = mk.data_ptr() if mk.numel() else None, mk.shape[1], mk.shape[2]
    imgs.n_images = len(masks)
    R = rois.shape[0] if num_rois is None else int(num_rois)
    out = torch.empty((rois.shape[0], m, m), device=rois.device, dtype=torch.float32)
    check(lib().mi355det_mask_targets(C.byref(imgs), ptr(rois), ptr(gt_index.to(torch.int64).contiguous()), R, m, ptr(out), stream_ptr()),
          "mask_targets")
    return out


def mask_loss(feat, w_logits, b_logits, labels, targets, valid, dfeat=None):
    """maskrcnn_loss fused with mask_fcn_logits on the label channel.  feat: bf16 deconvolution output (after ReLU) [rows, 14, 14, 1024] in
    sub-pixel order; labels [rows] int64; targets [rows, 28, 28]; valid = real rows (the rest is bucket padding).
    -> (loss [1], dfeat (gradient before the deconvolution's ReLU), dw [K, 256], db [K], dbias_deconv [256])."""
    rows = feat.shape[0]
    K = w_logits.shape[0]
    ld = feat.stride(2) if feat.dim() == 4 else feat.shape[-1]
    if feat.dtype != torch.bfloat16 or feat.shape[-1] != 1024 or w_logits.shape[1] != 256:
        raise ValueError("mask_loss: feat must be bf16 [rows, 14, 14, 1024], w_logits [K, 256]")
    dev = feat.device
    wl, bl = _f32c(w_logits), _f32c(b_logits)
    L = lib()
    wsb = L.mi355det_mask_loss_workspace(rows)
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    if dfeat is None:
        dfeat = torch.empty_like(feat)
    dw = torch.empty((K, 256), dtype=torch.float32, device=dev)
    db = torch.empty(K, dtype=torch.float32, device=dev)
    dbias = torch.empty(256, dtype=torch.float32, device=dev)
    check(L.mi355det_mask_loss(ptr(feat), ld, ptr(wl), ptr(bl), ptr(labels.to(torch.int64).contiguous()), ptr(_f32c(targets)), rows, int(valid), K,
                               ptr(loss), ptr(dfeat), ptr(dw), ptr(db), ptr(dbias), ptr(ws), wsb, stream_ptr()), "mask_loss")
    return loss, dfeat, dw, db, dbias


def mask_probs(feat, w_logits, b_logits, labels):
    """maskrcnn_inference: sigmoid of the label channel of mask_fcn_logits -> fp32 [rows, 28, 28]."""
    rows = feat.shape[0]
    ld = feat.stride(2) if feat.dim() == 4 else feat.shape[-1]
    probs = torch.empty((rows, 28, 28), dtype=torch.float32, device=feat.device)
    check(lib().mi355det_mask_probs(ptr(feat), ld, ptr(_f32c(w_logits)), ptr(_f32c(b_logits)), ptr(labels.to(torch.int64).contiguous()), rows,
                                    w_logits.shape[0], ptr(probs), stream_ptr()), "mask_probs")
    return probs


def mask_resize_nearest(masks, size, flip=False):
    """F.interpolate(masks[:, None].float(), size, mode='nearest')[:, 0].byte() for uint8 [G, h, w] (transform.py:54-60); with `flip`, of
    masks.flip(-1) (detection/transforms.py:38-39) without the flipped copy."""
    m = masks.to(torch.uint8).contiguous()
    if not m.is_cuda:
        raise ValueError("mask_resize_nearest needs CUDA/HIP tensors (no CPU fallback)")
    oh, ow = int(size[0]), int(size[1])
    out = torch.empty((m.shape[0], oh, ow), dtype=torch.uint8, device=m.device)
    if flip:
        check(lib().mi355det_mask_flip_resize_nearest(ptr(m), m.shape[0], m.shape[1], m.shape[2], ptr(out), oh, ow, 1, stream_ptr()),
              "mask_flip_resize_nearest")
    else:
        check(lib().mi355det_mask_resize_nearest(ptr(m), m.shape[0], m.shape[1], m.shape[2], ptr(out), oh, ow, stream_ptr()), "mask_resize_nearest")
    return out


# ------------------------------------------------------------------------------------ Keypoint R-CNN keypoint branch (csrc/keypoint_kernels.hip)
def _kp_batch(keypoints, what):
    """Per-image keypoints [G_b, K, 3] -> (fp32 [G, K, 3] on the device, int64 offsets [n + 1] on the device, K).  No host read."""
    if not keypoints:
        raise ValueError(f"{what}: no images")
    for kp in keypoints:
        if kp.dim() != 3 or kp.shape[2] != 3 or not kp.is_cuda:
            raise ValueError(f"{what}: keypoints must be CUDA [G, K, 3] per image")
    K = int(keypoints[0].shape[1])
    if any(int(kp.shape[1]) != K for kp in keypoints):
        raise ValueError(f"{what}: every image must have the same number of keypoints")
    offsets = [0]
    for kp in keypoints:
        offsets.append(offsets[-1] + int(kp.shape[0]))
    dev = keypoints[0].device
    return torch.cat([_f32c(kp) for kp in keypoints]), torch.tensor(offsets, dtype=torch.int64).to(dev, non_blocking=True), K


def keypoint_targets(keypoints, rois, gt_index, size=56, valid_rows=None):
    """keypoints_to_heatmap (roi_heads.py:186-219) for a whole batch in one launch: keypoints = per-image [G_b, K, 3]; rois [rows, 5] =
    (image, box); gt_index [rows] = matched gt inside the image -> (target int32 [rows, K], valid int32 [rows, K], count int32 [1], all on
    the device).  Rows >= valid_rows (bucket padding) are not valid."""
    rois = _f32c(rois)
    kp, offsets, K = _kp_batch(keypoints, "keypoint_targets")
    rows = rois.shape[0]
    dev = rois.device
    target = torch.empty((rows, K), dtype=torch.int32, device=dev)
    valid = torch.empty((rows, K), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().mi355det_keypoint_targets(ptr(kp), ptr(offsets), len(keypoints), ptr(rois), ptr(gt_index.to(torch.int64).contiguous()), rows,
                                          rows if valid_rows is None else int(valid_rows), K, int(size), ptr(target), ptr(valid), ptr(count),
                                          stream_ptr()), "keypoint_targets")
    return target, valid, count


def _kp_logits(what, z, num_keypoints):
    if z.dtype != torch.float32 or z.dim() != 4 or tuple(z.shape[1:3]) != (14, 14) or z.shape[3] % 4 or z.stride(3) != 1 or not z.is_cuda:
        raise ValueError(f"{what}: logits must be CUDA fp32 [rows, 14, 14, 4 * KP] (sub-pixel layout)")
    kp = z.shape[3] // 4
    if not 1 <= num_keypoints <= kp:
        raise ValueError(f"{what}: {num_keypoints} keypoints do not fit {kp} padded channels")
    if z.stride(1) != 14 * z.stride(2) or z.stride(0) != 196 * z.stride(2):
        raise ValueError(f"{what}: logits must be dense over the pixels")
    return kp, z.stride(2)


def keypoint_heatmaps(z, num_keypoints):
    """The predictor's bilinear x2: sub-pixel logits fp32 [rows, 14, 14, 4 * KP] -> fp32 [rows, K, 56, 56]."""
    kp, ld = _kp_logits("keypoint_heatmaps", z, num_keypoints)
    out = torch.empty((z.shape[0], num_keypoints, 56, 56), dtype=torch.float32, device=z.device)
    check(lib().mi355det_keypoint_heatmaps(ptr(z), ld, kp, z.shape[0], num_keypoints, ptr(out), stream_ptr()), "keypoint_heatmaps")
    return out


def keypoint_loss(z, target, valid, count, want_f32_grad=False, want_terms=False):
    """keypointrcnn_loss (roi_heads.py:330-357) fused with the bilinear x2.  z: sub-pixel logits fp32 [rows, 14, 14, 4 * KP]; target, valid,
    count: what keypoint_targets returned -> (loss [1], dz bf16 like z, dbias [K]); with want_f32_grad also the gradient before its rounding
    to bf16, fp32 [rows, K, 28, 28]; with want_terms also the per-pair loss terms lse - logit[target], fp32 [rows, K] (0 where the pair is not
    valid; the loss is their sum over count), read out of the kernel's workspace.  Bit-identical from run to run."""
    K = target.shape[1]
    kp, ld = _kp_logits("keypoint_loss", z, K)
    rows = z.shape[0]
    if tuple(target.shape) != (rows, K) or tuple(valid.shape) != (rows, K) or target.dtype != torch.int32 or valid.dtype != torch.int32:
        raise ValueError("keypoint_loss: target and valid must be int32 [rows, K]")
    dev = z.device
    L = lib()
    wsb = L.mi355det_keypoint_loss_workspace(rows, K)
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dz = torch.empty(z.shape[:3] + (ld,), dtype=torch.bfloat16, device=dev)[..., :z.shape[3]]
    dbias = torch.empty(K, dtype=torch.float32, device=dev)
    d32 = torch.empty((rows, K, 28, 28), dtype=torch.float32, device=dev) if want_f32_grad else None
    check(L.mi355det_keypoint_loss(ptr(z), ld, kp, rows, K, ptr(target.contiguous()), ptr(valid.contiguous()), ptr(count), ptr(loss), ptr(dz),
                                   ptr(d32), ptr(dbias), ptr(ws), wsb, stream_ptr()), "keypoint_loss")
    out = (loss, dz, dbias) + ((d32,) if want_f32_grad else ())
    if want_terms:
        out += (ws[:rows * K * 8].view(torch.float32).view(rows, K, 2)[..., 0].clone(),)
    return out


def heatmaps_to_keypoints(maps, rois):
    """heatmaps_to_keypoints (roi_heads.py:274-327) for all RoIs in one launch, no host read: maps fp32 [rows, K, 56, 56]; rois [rows, 4]
    boxes or [rows, 5] (image, box) -> (xy [rows, K, 3], scores [rows, K])."""
    maps, rois = _f32c(maps), _f32c(rois)
    if maps.dim() != 4 or tuple(maps.shape[2:]) != (56, 56) or not maps.is_cuda:
        raise ValueError("heatmaps_to_keypoints: maps must be CUDA fp32 [rows, K, 56, 56]")
    rows, K = maps.shape[0], maps.shape[1]
    if rois.dim() != 2 or rois.shape[0] != rows or rois.shape[1] not in (4, 5):
        raise ValueError("heatmaps_to_keypoints: rois must be [rows, 4] or [rows, 5]")
    xy = torch.empty((rows, K, 3), dtype=torch.float32, device=maps.device)
    scores = torch.empty((rows, K), dtype=torch.float32, device=maps.device)
    check(lib().mi355det_heatmaps_to_keypoints(ptr(maps), ptr(rois), rois.shape[1], rows, K, ptr(xy), ptr(scores), stream_ptr()),
          "heatmaps_to_keypoints")
    return xy, scores


def _device_bytes(what, **tensors):
    for name, (t, dtype) in tensors.items():
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {dtype} CUDA/HIP tensor (no CPU fallback)")


def _need_device(what, *tensors):
    """The refusal of the run-length and evaluation ops: every operand named here is a tensor on the device."""
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{what} needs CUDA/HIP tensors (no CPU fallback)")


def _emit_buffers(n, total, capacity, dev, out=None):
    """What an emit pass of "count, one host read, emit" writes for n masks with `total` counts: (counts int32 [cap], area int64 [n],
    bbox int32 [n, 4], cap).  cap = `capacity` or the exact size; `out` = the caller's counts buffer in place of a new one."""
    cap = int(total) if capacity is None else int(capacity)
    counts = torch.empty(max(cap, 0), dtype=torch.int32, device=dev) if out is None else out
    return counts, torch.empty(n, dtype=torch.int64, device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev), cap


def _no_runs(dev):
    """(counts, area, bbox) of no masks."""
    return _emit_buffers(0, 0, None, dev)[:3]


def yolo_ingest_u8(packed, table, table_dev, taps_dev, lut, size, out=None):
    """mi355det_yolo_ingest_u8: OpenCV's 8-bit bicubic resize to size x size, / 255 and normalise of a packed batch of uint8 images in one
    launch (the rule: include/mi355det.h).  packed: uint8 [bytes] on the device; table: a host (_lib.YoloImage * n) array, table_dev: its
    bytes on the device (uint8); taps_dev: the (s, w0..w3) entries of both axes as bytes on the device (uint8, 12 each); lut: fp32 [3, 256]
    on the device.  Returns fp32 [n, 3, size, size]."""
    n, size = len(table), int(size)
    _device_bytes("yolo_ingest_u8", packed=(packed, torch.uint8), table_dev=(table_dev, torch.uint8), taps_dev=(taps_dev, torch.uint8),
                  lut=(lut, torch.float32))
    if table_dev.numel() != C.sizeof(table) or taps_dev.numel() % C.sizeof(_lib.CubicTap) or lut.numel() != 768:
        raise ValueError("yolo_ingest_u8: table_dev, taps_dev or lut has the wrong size")
    if out is None:
        out = torch.empty((n, 3, size, size), dtype=torch.float32, device=packed.device)
    elif tuple(out.shape) != (n, 3, size, size):
        raise ValueError("yolo_ingest_u8: out must be [n, 3, size, size]")
    _device_bytes("yolo_ingest_u8", out=(out, torch.float32))
    check(_lib.lib().mi355det_yolo_ingest_u8(ptr(packed), packed.numel(), C.cast(table, C.c_void_p), ptr(table_dev), n, ptr(taps_dev),
                                             taps_dev.numel() // C.sizeof(_lib.CubicTap), ptr(lut), ptr(out), size, stream_ptr()), "yolo_ingest_u8")
    return out


def yolo_targets(boxes, area, box_offsets_dev, table_dev, n):
    """mi355det_yolo_targets: all boxes of a batch in one launch.  boxes float64 [G, 4] (xmin, ymin, w, h) and area float64 [G] on the
    device, box_offsets_dev int64 [n + 1], table_dev as for `yolo_ingest_u8`.  Returns (bbox fp32 [G, 4] relative xcycwh, flipped where the
    image is, area / (h * w) float64 [G])."""
    _device_bytes("yolo_targets", boxes=(boxes, torch.float64), area=(area, torch.float64), box_offsets_dev=(box_offsets_dev, torch.int64),
                  table_dev=(table_dev, torch.uint8))
    g = int(area.numel())
    if tuple(boxes.shape) != (g, 4) or box_offsets_dev.numel() != n + 1 or table_dev.numel() != n * C.sizeof(_lib.YoloImage):
        raise ValueError("yolo_targets: boxes [G, 4], area [G], box_offsets [n + 1] and a table of n images are expected")
    bbox = torch.empty((g, 4), dtype=torch.float32, device=boxes.device)
    rel = torch.empty((g,), dtype=torch.float64, device=boxes.device)
    check(_lib.lib().mi355det_yolo_targets(ptr(boxes), ptr(area), g, ptr(box_offsets_dev), ptr(table_dev), int(n), ptr(bbox), ptr(rel), stream_ptr()),
          "yolo_targets")
    return bbox, rel


def paste_masks(masks, boxes, img_shape, padding=1):
    """paste_masks_in_image (roi_heads.py:517-537): masks [D, 1, M, M] fp32, boxes [D, 4] -> [D, 1, H, W] fp32."""
    m = _f32c(masks)
    D, M = m.shape[0], m.shape[-1]
    H, W = int(img_shape[0]), int(img_shape[1])
    out = torch.empty((D, 1, H, W), dtype=torch.float32, device=m.device)
    check(lib().mi355det_paste_masks(ptr(m), ptr(_f32c(boxes)), D, M, int(padding), H, W, ptr(out), stream_ptr()), "paste_masks")
    return out


def _mask_rle(dense, masks, boxes, D, M, padding, H, W, threshold, dev, capacity=None):
    """count -> ONE host read of the offsets -> emit into exactly sized counts (mi355det_mask_rle_count / _emit)."""
    from .rle import RLEBatch
    L = lib()
    if D == 0:
        # the argument checks still run (no launch: num_masks == 0 succeeds)
        check(L.mi355det_mask_rle_count(ptr(dense), ptr(masks), ptr(boxes), 0, M, padding, H, W, threshold, None, None, 0, stream_ptr()), "mask_rle_count")
        counts, area, bbox = _no_runs(dev)
        return RLEBatch((H, W), counts, [0], area, bbox)
    nbytes = L.mi355det_mask_rle_workspace(D, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    run_offsets = torch.empty(D + 1, dtype=torch.int64, device=dev)
    src = (ptr(dense), ptr(masks), ptr(boxes), D, M, padding, H, W, threshold)
    check(L.mi355det_mask_rle_count(*src, ptr(run_offsets), ptr(ws), nbytes, stream_ptr()), "mask_rle_count")
    offsets = run_offsets.tolist()                         # the one host read: the strings are built from these numbers anyway
    total = offsets[-1]
    counts, area, bbox, cap = _emit_buffers(D, total, capacity, dev)
    check(L.mi355det_mask_rle_emit(*src, ptr(run_offsets), total, ptr(counts), cap, ptr(area), ptr(bbox), ptr(ws), nbytes, stream_ptr()),
          "mask_rle_emit")
    return RLEBatch((H, W), counts, offsets, area, bbox)


def mask_rle_dense(masks, threshold=0.5, capacity=None):
    """`masks > threshold` as COCO run lengths (coco_eval.py:117-125 without the host bitmap): masks fp32 [D, H, W] or [D, 1, H, W] ->
    RLEBatch.  `capacity` (elements of the counts buffer) defaults to the exact size."""
    m = _f32c(masks)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3:
        raise ValueError("mask_rle_dense: masks must be [D, H, W] or [D, 1, H, W]")
    D, H, W = (int(v) for v in m.shape)
    return _mask_rle(m, None, None, D, 1, 0, H, W, float(threshold), m.device, capacity)


def mask_rle_paste(masks, boxes, img_shape, padding=1, threshold=0.5, capacity=None):
    """The run lengths of `paste_masks(masks, boxes, img_shape, padding) > threshold` straight from the [D, 1, M, M] probabilities and the
    boxes: the [D, H, W] mask is never written (threshold >= 0).  -> RLEBatch."""
    m = _f32c(masks)
    D, M = int(m.shape[0]), int(m.shape[-1])
    b = _f32c(boxes)
    if b.shape != (D, 4):
        raise ValueError("mask_rle_paste: boxes must be [D, 4]")
    H, W = int(img_shape[0]), int(img_shape[1])
    return _mask_rle(None, m, b, D, M, int(padding), H, W, float(threshold), m.device, capacity)


# ---- run lengths from counts strings (csrc/rle_string_kernels.hip; the mask store on top of these is cocoeval._MaskStore)
RLESTR_RANGE, RLESTR_SIZE, RLESTR_ALPHABET, RLESTR_LONG, RLESTR_OPEN, RLESTR_INT32, RLESTR_NEGATIVE, RLESTR_SUM = (1 << b for b in range(8))
RLESTR_PARSE = RLESTR_ALPHABET | RLESTR_LONG | RLESTR_OPEN | RLESTR_INT32        # what mi355det_rle_from_string refuses


def _rle_strings_operands(what, packed, str_offsets, str_offsets_dev, sizes):
    import numpy as np
    _need_device(what, packed, str_offsets_dev, sizes)
    host = np.ascontiguousarray(str_offsets, dtype=np.int64).reshape(-1)
    n = int(host.shape[0]) - 1
    if packed.dtype != torch.uint8 or str_offsets_dev.dtype != torch.int64 or sizes.dtype != torch.int32:
        raise ValueError(f"{what}: packed must be uint8, str_offsets_dev int64 and sizes int32")
    if n < 0 or int(str_offsets_dev.numel()) != n + 1 or tuple(sizes.shape) != (n, 2):
        raise ValueError(f"{what}: str_offsets [n + 1] on both sides and sizes [n, 2]")
    return packed.contiguous(), host, str_offsets_dev.contiguous(), sizes.contiguous(), n


def rle_strings_count(packed, str_offsets, str_offsets_dev, sizes):
    """mi355det_rle_strings_count: packed uint8 [bytes] on the device, str_offsets int64 [n + 1] on the host and its device copy, sizes int32
    [n, 2] on the device -> (table int64 [n + 2] on the device: the run offsets [n + 1], then the number of masks with a status; status uint8
    [n] on the device).  One host read of `table` gives what sizes the counts and whether any mask was refused."""
    packed, host, d_off, sizes, n = _rle_strings_operands("rle_strings_count", packed, str_offsets, str_offsets_dev, sizes)
    table = torch.empty(n + 2, dtype=torch.int64, device=packed.device)
    status = torch.empty(n, dtype=torch.uint8, device=packed.device)
    check(lib().mi355det_rle_strings_count(ptr(packed), int(packed.numel()), host.ctypes.data_as(C.c_void_p), ptr(d_off), ptr(sizes), n,
                                           ptr(table), ptr(status), C.c_void_p(table.data_ptr() + 8 * (n + 1)), stream_ptr()),
          "rle_strings_count")
    return table, status


def rle_strings_emit(packed, str_offsets_dev, sizes, run_offsets, total_runs, capacity=None):
    """mi355det_rle_strings_emit after rle_strings_count on the same operands: run_offsets int64 [n + 1] on the device, total_runs the
    host's copy of its last entry -> (counts int32 [total_runs], area int64 [n], bbox int32 [n, 4]) on the device."""
    _need_device("rle_strings_emit", packed, str_offsets_dev, sizes, run_offsets)
    n = int(sizes.shape[0])
    if run_offsets.dtype != torch.int64 or int(run_offsets.numel()) < n + 1 or int(str_offsets_dev.numel()) != n + 1:
        raise ValueError("rle_strings_emit: run_offsets and str_offsets_dev must be int64 [n + 1]")
    counts, area, bbox, cap = _emit_buffers(n, total_runs, capacity, packed.device)
    check(lib().mi355det_rle_strings_emit(ptr(packed), int(packed.numel()), ptr(str_offsets_dev), ptr(sizes), n, ptr(run_offsets),
                                          int(total_runs), ptr(counts), cap, ptr(area), ptr(bbox), stream_ptr()), "rle_strings_emit")
    return counts, area, bbox


def rle_strings(packed, str_offsets, sizes, device=None, mark=None):
    """The masks of a results file from their `counts` strings (rle.pack_strings): packed uint8 [bytes], str_offsets int64 [n + 1] and
    sizes [n, 2] = [h, w] as host arrays -> (counts int32, run offsets as a host int64 array [n + 1], area int64 [n], bbox int32 [n, 4],
    status): everything else on the device; status is None when every mask is valid, else a host uint8 array [n] of RLESTR_* bits (the
    other results are then of no use).  Two uploads (the bytes; the offsets and sizes as one table), count, ONE host read, emit.
    `mark(name)` is called after the stages "upload", "count" and "emit" (tools/bench_lvissegm.py times them with it)."""
    import numpy as np
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError("rle_strings needs a CUDA/HIP device (no CPU fallback)")
    mark = mark or (lambda name: None)
    host_off = np.ascontiguousarray(str_offsets, dtype=np.int64).reshape(-1)
    n = int(host_off.shape[0]) - 1
    sz = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 2)
    if n < 0 or sz.shape[0] != n:
        raise ValueError("rle_strings: str_offsets [n + 1] and sizes [n, 2]")
    table = np.empty(2 * n + 1, np.int64)                  # the offsets, then the sizes: two int32 fill one int64 slot
    table[:n + 1] = host_off
    table[n + 1:].view(np.int32)[:] = sz.reshape(-1)
    d_table = torch.from_numpy(table).to(dev)
    d_bytes = torch.from_numpy(np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1)).to(dev)
    d_off, d_sz = d_table[:n + 1], d_table[n + 1:].view(torch.int32).view(n, 2)
    mark("upload")
    out, status = rle_strings_count(d_bytes, host_off, d_off, d_sz)
    mark("count")
    host = out.cpu().numpy()                               # the one host read: the offsets size the counts, the last entry tells of refusals
    runs, bad = host[:n + 1], int(host[n + 1])
    counts, area, bbox = rle_strings_emit(d_bytes, d_off, d_sz, out, int(runs[-1]))
    mark("emit")
    return counts, runs, area, bbox, (status.cpu().numpy() if bad else None)


# ---- mask boundaries as run lengths (csrc/boundary_kernels.hip; include/mi355det.h "Mask boundaries as run lengths")
def _host_table(t, dtype, shape, what):
    """An operand the host checks read: a host array as it is, a device tensor through one copy.  dtype int32: wider integers are clipped
    into its range first (what is out of range stays out of range for the checks)."""
    import numpy as np
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if dtype == np.int32 and a.dtype != np.int32:
        a = np.asarray(a, np.int64).clip(-2 ** 31, 2 ** 31 - 1)
    a = np.ascontiguousarray(a, dtype=dtype)
    try:
        return a.reshape(shape)
    except ValueError:
        raise ValueError(f"rle_boundary: {what} must have shape {list(shape)}") from None


class BoundaryPlan:
    """The operands of mi355det_rle_boundary_count / _emit, checked and laid out by mi355det_rle_boundary_plan: the host tables, their device
    copies, the chunks and one workspace for all of them.  count() -> run offsets int64 [n + 1] on the device; emit(run_offsets, total) ->
    (counts, area, bbox).  ops.rle_boundary is plan, count, one host read, emit; tools/bench_boundary.py times the two passes apart."""

    def __init__(self, counts, runs, sizes, dilation, boxes, index=None, budget_bytes=1 << 30):
        import numpy as np
        _need_device("rle_boundary", counts)
        for t in (runs, sizes, dilation, boxes, index):
            if torch.is_tensor(t) and not t.is_cuda:
                raise ValueError("rle_boundary needs CUDA/HIP tensors (no CPU fallback); tables for the host checks are numpy arrays or lists")
        if counts.dtype != torch.int32:
            raise ValueError("rle_boundary: counts must be int32")
        self.dev, self.counts = counts.device, counts.contiguous()
        h_runs = _host_table(runs, np.int64, (-1,), "runs")
        num_src = int(h_runs.shape[0]) - 1
        if num_src < 0:
            raise ValueError("rle_boundary: runs must hold masks + 1 entries")
        h_index = None if index is None else _host_table(index, np.int64, (-1,), "index")
        self.n = n = num_src if h_index is None else int(h_index.shape[0])
        geom = np.empty((n, 7), np.int32)
        geom[:, 0:2] = _host_table(sizes, np.int32, (n, 2), "sizes")
        dil = np.asarray(dilation.detach().cpu().numpy() if torch.is_tensor(dilation) else dilation)
        if dil.dtype.kind not in "iu":
            raise ValueError("rle_boundary: the dilation must be an integer (rle.boundary_dilation)")
        dil = dil.astype(np.int64).clip(-1, 2 ** 31 - 1).reshape(-1)
        if dil.size not in (1, n):
            raise ValueError("rle_boundary: one dilation for all masks, or one per mask")
        geom[:, 2] = dil if dil.size == n else dil[0]
        geom[:, 3:7] = _host_table(boxes, np.int32, (n, 4), "boxes")
        hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        slices, starts, need = np.zeros(max(n, 1), np.int64), np.zeros(n + 1, np.int64), np.zeros(1, np.int64)
        chunks = int(lib().mi355det_rle_boundary_plan(hp(h_runs), num_src, int(self.counts.numel()), hp(h_index), hp(geom), n, int(budget_bytes),
                                                      hp(slices), hp(starts), hp(need)))
        if chunks < 0:
            check(chunks, "rle_boundary_plan")
        self.chunks = [(int(starts[j]), int(starts[j + 1] - starts[j])) for j in range(chunks)]
        up = lambda a: torch.from_numpy(a).to(self.dev)
        d_runs = runs.to(torch.int64).contiguous().reshape(-1) if torch.is_tensor(runs) else up(h_runs)
        d_index = None if h_index is None else (index.to(torch.int64).contiguous().reshape(-1) if torch.is_tensor(index) else up(h_index))
        d_geom, d_slices = up(geom), up(slices)
        self.nbytes = int(need[0])
        self.ws = torch.empty(max(self.nbytes, 8), dtype=torch.uint8, device=self.dev)
        self._keep = (h_runs, h_index, geom, slices, d_runs, d_index, d_geom, d_slices)
        self._tables = (ptr(self.counts), int(self.counts.numel()), hp(h_runs), ptr(d_runs), num_src, hp(h_index), ptr(d_index), hp(geom),
                        ptr(d_geom), hp(slices), ptr(d_slices), n)

    def count(self):
        i64 = dict(dtype=torch.int64, device=self.dev)
        num_runs = torch.empty(self.n, **i64)
        for first, num in self.chunks:
            check(lib().mi355det_rle_boundary_count(*self._tables, first, num, ptr(num_runs), ptr(self.ws), self.nbytes, stream_ptr()),
                  "rle_boundary_count")
        return torch.cat([torch.zeros(1, **i64), torch.cumsum(num_runs, 0)])

    def emit(self, run_offsets, total):
        out, area, bbox, cap = _emit_buffers(self.n, total, None, self.dev)
        for first, num in self.chunks:
            check(lib().mi355det_rle_boundary_emit(*self._tables, first, num, ptr(run_offsets), cap, ptr(out), cap, ptr(area),
                                                   ptr(bbox), ptr(self.ws), self.nbytes, stream_ptr()), "rle_boundary_emit")
        return out, area, bbox


def rle_boundary(counts, runs, sizes, dilation, boxes, index=None, budget_bytes=1 << 30):
    """The boundaries `mask & ~eroded` of n masks as run lengths (mi355det_rle_boundary_*): counts int32 on the device and runs [masks + 1] as
    the run-length ops give them, sizes [n, 2] = [h, w], dilation (an int for all, or [n]; rle.boundary_dilation), boxes [n, 4] = the masks'
    tight boxes [x, y, w, h] and index [n] or None (output mask k is the boundary of mask index[k]) ->
    (counts int32, run offsets as a host int64 array [n + 1], area int64 [n], bbox int32 [n, 4]); all but the offsets on the device.
    runs, sizes, dilation, boxes and index are read on the host (they size the scratch and are checked there): host arrays cost nothing,
    device tensors one copy each.  Then count -> ONE host read of the run offsets -> emit; both passes go over the masks in chunks whose
    scratch stays within `budget_bytes` (one mask at least), and the result does not depend on the chunking."""
    plan = BoundaryPlan(counts, runs, sizes, dilation, boxes, index, budget_bytes)
    run_offsets = plan.count()
    offsets = run_offsets.cpu().numpy()                    # the one host read: it sizes the counts
    out, area, bbox = plan.emit(run_offsets, int(offsets[-1]))
    return out, offsets, area, bbox


# ---- COCO polygons as run lengths, and run lengths as bitmaps (csrc/poly_kernels.hip; the readers on top are object_detectors_amd/polygons.py)
POLY_MAX_COORD = float(1 << 24)


def _poly_tables(xy, poly_offsets, ann_offsets, sizes):
    """The host side of poly_rle's contract: every refusal is a ValueError before anything reaches the device."""
    import numpy as np
    po = np.ascontiguousarray(poly_offsets, dtype=np.int64).reshape(-1)
    ao = np.ascontiguousarray(ann_offsets, dtype=np.int64).reshape(-1)
    sz = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1, 2)
    if po.size < 1 or po[0] != 0 or ao.size < 1 or ao[0] != 0:
        raise ValueError("poly_rle: offsets must begin with 0")
    if (np.diff(po) < 3).any():
        raise ValueError("poly_rle: a polygon needs at least 3 points")
    if (np.diff(ao) < 0).any() or ao[-1] != po.size - 1:
        raise ValueError("poly_rle: ann_offsets must rise from 0 to the number of polygons")
    if sz.shape[0] != ao.size - 1:
        raise ValueError("poly_rle: sizes must be [number of annotations, 2]")
    if (sz < 1).any() or (sz[:, 0] * sz[:, 1] >= (1 << 31)).any():
        raise ValueError("poly_rle: every size needs h, w >= 1 and h*w < 2^31")
    if po.size - 1 >= (1 << 31) or ao.size - 1 >= (1 << 31):
        raise ValueError("poly_rle: too many polygons")
    n = int(xy.numel()) if torch.is_tensor(xy) else int(np.asarray(xy).size)
    if n != 2 * int(po[-1]):
        raise ValueError("poly_rle: xy must hold 2 coordinates per point of poly_offsets")
    if torch.is_tensor(xy):
        bad = n > 0 and not bool((torch.isfinite(xy) & (xy.abs() < POLY_MAX_COORD)).all())
    else:
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
        bad = n > 0 and not bool((np.isfinite(xy) & (np.abs(xy) < POLY_MAX_COORD)).all())
    if bad:
        raise ValueError("poly_rle: every coordinate must be finite with |c| < 2^24")
    return xy, po, ao, sz.astype(np.int32)


def poly_rle(xy, poly_offsets, ann_offsets, sizes, capacity=None, device=None, mark=None, out=None):
    """pycocotools merge(frPyObjects(polygons, h, w)) of many annotations at once (mi355det_poly_*): xy float64 [2 * points] (host array, or
    a tensor already on the device), poly_offsets [NP + 1] in points, ann_offsets [A + 1] in polygons and sizes [A, 2] = [h, w] on the host
    -> (counts int32 on the device, run_offsets host list [A + 1], area int64 [A], bbox int32 [A, 4]).  Two host reads: the point offsets
    (they size the keys) and the run offsets (they size the counts).  `capacity` (elements of the counts buffer) defaults to the exact size; `out` is a counts buffer of the caller's;
    `mark(name)` is called after the stages "points", "sort", "events" and "runs" (tools/bench_poly_rle.py times them with it)."""
    import numpy as np
    xy, po, ao, sz = _poly_tables(xy, poly_offsets, ann_offsets, sizes)
    NP, A = int(po.size) - 1, int(ao.size) - 1
    dev = xy.device if torch.is_tensor(xy) and xy.is_cuda else torch.device("cuda" if device is None else device)
    mark = mark or (lambda name: None)
    i64 = dict(dtype=torch.int64, device=dev)
    if A == 0:
        counts, area, bbox = _no_runs(dev)
        return counts, [0], area, bbox
    L = lib()
    d_xy = torch.as_tensor(xy, dtype=torch.float64).to(dev).contiguous().reshape(-1)
    d_po, d_ao, d_sz = torch.from_numpy(po).to(dev), torch.from_numpy(ao).to(dev), torch.from_numpy(sz).to(dev)
    keys = events = pt_off = tog_off = None
    if NP > 0:
        tables = (ptr(d_po), ptr(d_ao), ptr(d_sz), NP, A)
        pt_off = torch.empty(NP + 1, **i64)
        check(L.mi355det_poly_points_count(ptr(d_xy), *tables, ptr(pt_off), stream_ptr()), "poly_points_count")
        pts = pt_off.cpu().numpy()                         # host read 1 of 2
        total = int(pts[-1])
        keys = torch.empty(total, **i64)
        check(L.mi355det_poly_points_emit(ptr(d_xy), *tables, ptr(pt_off), total, ptr(keys), total, stream_ptr()), "poly_points_emit")
        mark("points")
        keys = torch.sort(keys).values
        mark("sort")
        # the parts of annotations with two or more parts become coverage events; their slots are sized by their point counts
        parts = np.diff(ao)
        multi = np.repeat(parts >= 2, parts)
        slots = np.where(multi, np.diff(pts), 0)
        base = np.where(multi, np.cumsum(slots) - slots, -1).astype(np.int64)
        cap_ev = int(slots.sum())
        events = torch.empty(cap_ev, **i64)
        tog_off = torch.empty(NP + 1, **i64)
        check(L.mi355det_poly_events(ptr(keys), ptr(pt_off), ptr(d_ao), ptr(d_sz), ptr(torch.from_numpy(base).to(dev)), NP, A, ptr(events),
                                     cap_ev, ptr(tog_off), stream_ptr()), "poly_events")
        if cap_ev:
            events = torch.sort(events).values
        mark("events")
    src = (ptr(keys), ptr(pt_off), ptr(events), ptr(tog_off), ptr(d_ao), ptr(d_sz), NP, A)
    run_offsets = torch.empty(A + 1, **i64)
    check(L.mi355det_poly_runs_count(*src, ptr(run_offsets), stream_ptr()), "poly_runs_count")
    offsets = run_offsets.tolist()                         # host read 2 of 2
    total = offsets[-1]
    # the caller's buffer: nothing is written at or past `capacity`
    if out is not None and (out.dtype != torch.int32 or out.device != d_ao.device or not out.is_contiguous()
                            or out.numel() < (total if capacity is None else int(capacity))):
        raise ValueError("poly_rle: out must be a contiguous int32 device tensor of at least `capacity` elements")
    counts, area, bbox, cap = _emit_buffers(A, total, capacity, dev, out)
    check(L.mi355det_poly_runs_emit(*src, ptr(run_offsets), total, ptr(counts), cap, ptr(area), ptr(bbox), stream_ptr()), "poly_runs_emit")
    mark("runs")
    return counts, offsets, area, bbox


def mask_rle_decode(batch_or_counts, run_offsets=None, size=None):
    """Run lengths -> bitmaps uint8 [D, H, W] on the device (mi355det_rle_decode): an RLEBatch whose counts are on the device, or device
    counts int32 with run_offsets [D + 1] (host list or tensor) and size = (H, W).  = RLEBatch.decode() without the host."""
    from .rle import RLEBatch
    if isinstance(batch_or_counts, RLEBatch):
        counts, run_offsets, size = batch_or_counts.counts, batch_or_counts.offsets, batch_or_counts.size
    else:
        counts = batch_or_counts
    if run_offsets is None or size is None:
        raise ValueError("mask_rle_decode: counts need run_offsets and size")
    if not torch.is_tensor(counts) or not counts.is_cuda:
        raise ValueError("mi355det ops need CUDA/HIP tensors (no CPU fallback)")
    H, W = int(size[0]), int(size[1])
    if not torch.is_tensor(run_offsets):
        off = [int(o) for o in run_offsets]
        if not off or off[0] != 0 or off[-1] > int(counts.shape[0]) or any(b < a for a, b in zip(off, off[1:])):
            raise ValueError("mask_rle_decode: run_offsets must rise from 0 and stay within counts")
        run_offsets = torch.tensor(off, dtype=torch.int64)
    run_offsets = run_offsets.to(device=counts.device, dtype=torch.int64).contiguous()
    D = int(run_offsets.shape[0]) - 1
    if D < 0:
        raise ValueError("mask_rle_decode: run_offsets must hold D + 1 entries")
    c = counts.to(torch.int32).contiguous()
    out = torch.empty((D, H, W), dtype=torch.uint8, device=c.device)
    check(lib().mi355det_rle_decode(ptr(c), ptr(run_offsets), D, H, W, ptr(out), stream_ptr()), "rle_decode")
    return out


# ---- COCO evaluation (csrc/cocoeval_kernels.hip; the evaluator on top of these is object_detectors_amd/cocoeval.py)
def _f64c(t, dev):
    return torch.as_tensor(t, dtype=torch.float64, device=dev).contiguous()


def coco_iou(dt_offsets, gt_offsets, iou_offsets, iou_size, dt_boxes, gt_boxes, gt_crowd, rle=None):
    """mi355det_coco_iou over ragged groups: offsets int64 [NG + 1] on the device, boxes float64 [*, 4] as [x, y, w, h], gt_crowd uint8 ->
    float64 [iou_size].  `rle` switches to run-length mode: a dict with dt / gt = (counts int32, runs int64 [masks + 1], index int64 or None)
    on the device and dt_sizes / gt_sizes = host int32 [NG, 2]; the boxes are then the masks' tight boxes."""
    import numpy as np
    dev = dt_boxes.device
    _need_device("coco_iou", dt_boxes)
    ng = int(dt_offsets.shape[0]) - 1
    nd, ngt = int(dt_boxes.shape[0]), int(gt_boxes.shape[0])
    out = torch.empty(int(iou_size), dtype=torch.float64, device=dev)
    if rle is None:
        side = (None, None, None, 0, 0)
        args = side + side + (None, None)
        keep = ()
    else:
        def one(s):
            counts, runs, index = s
            return (ptr(counts), ptr(runs), ptr(index), int(runs.shape[0]) - 1, int(counts.shape[0]))
        sizes = [np.ascontiguousarray(rle[k], dtype=np.int32).reshape(-1, 2) for k in ("dt_sizes", "gt_sizes")]
        if any(s.shape[0] != ng for s in sizes):
            raise ValueError("coco_iou: one [h, w] per group and side")
        args = one(rle["dt"]) + one(rle["gt"]) + tuple(s.ctypes.data_as(C.c_void_p) for s in sizes)
        keep = sizes
    check(lib().mi355det_coco_iou(0 if rle is None else 1, ng, ptr(dt_offsets), ptr(gt_offsets), ptr(iou_offsets), nd, ngt, int(iou_size),
                                  ptr(dt_boxes), ptr(gt_boxes), ptr(gt_crowd), *args, ptr(out), stream_ptr()), "coco_iou")
    del keep
    return out


def _match(entry, what, dt_offsets, gt_offsets, iou_offsets, iou, dt_area, gt_area, flags, iou_thrs, area_rngs):
    """The match entries: `flags` = the uint8 operands between gt_area and iou_thrs (gt_crowd; for LVIS gt_flag, group_not_exhaustive)."""
    dev = iou.device
    ng, nd, ngt = int(dt_offsets.shape[0]) - 1, int(dt_area.shape[0]), int(gt_area.shape[0])
    T, A = int(iou_thrs.shape[0]), int(area_rngs.shape[0])
    dt_match = torch.zeros((A, T, nd), dtype=torch.int32, device=dev)
    dt_ignore = torch.zeros((A, T, nd), dtype=torch.uint8, device=dev)
    gt_match = torch.zeros((A, T, ngt), dtype=torch.int32, device=dev)
    gt_ignore = torch.zeros((A, ngt), dtype=torch.uint8, device=dev)
    check(entry(ng, ptr(dt_offsets), ptr(gt_offsets), ptr(iou_offsets), nd, ngt, int(iou.shape[0]), ptr(iou), ptr(dt_area), ptr(gt_area),
                *[ptr(f) for f in flags], ptr(iou_thrs), T, ptr(area_rngs), A, ptr(dt_match), ptr(dt_ignore), ptr(gt_match), ptr(gt_ignore),
                stream_ptr()), what)
    return dt_match, dt_ignore, gt_match, gt_ignore


def coco_match(dt_offsets, gt_offsets, iou_offsets, iou, dt_area, gt_area, gt_crowd, iou_thrs, area_rngs):
    """mi355det_coco_match -> dt_match int32 [A, T, ND], dt_ignore uint8 [A, T, ND], gt_match int32 [A, T, NG], gt_ignore uint8 [A, NG]."""
    _need_device("coco_match", iou)
    return _match(lib().mi355det_coco_match, "coco_match", dt_offsets, gt_offsets, iou_offsets, iou, dt_area, gt_area, [gt_crowd], iou_thrs,
                  area_rngs)


def lvis_match(dt_offsets, gt_offsets, iou_offsets, iou, dt_area, gt_area, gt_flag, group_not_exhaustive, iou_thrs, area_rngs):
    """mi355det_lvis_match (the match under LVISEval's rules: gt_flag uint8 [NG] = the annotations' ignore flags, group_not_exhaustive uint8
    [groups]) -> the four arrays of coco_match, same layouts."""
    _need_device("lvis_match", iou, group_not_exhaustive)
    if group_not_exhaustive.dtype != torch.uint8 or int(group_not_exhaustive.shape[0]) != int(dt_offsets.shape[0]) - 1:
        raise ValueError("lvis_match: group_not_exhaustive must be uint8, one flag per group")
    return _match(lib().mi355det_lvis_match, "lvis_match", dt_offsets, gt_offsets, iou_offsets, iou, dt_area, gt_area,
                  [gt_flag, group_not_exhaustive.contiguous()], iou_thrs, area_rngs)


def coco_oks(dt_offsets, gt_offsets, iou_offsets, iou_size, dt_kp, gt_kp, gt_boxes, gt_area, vars):
    """mi355det_coco_oks over ragged groups (the offsets and the output layout of coco_iou): dt_kp float64 [ND, K, 2] (x, y), gt_kp float64
    [NG, K, 3] (x, y, v), gt_boxes float64 [NG, 4] as [x, y, w, h], gt_area float64 [NG], vars float64 [K] = (2 * sigma)^2 -> the object
    keypoint similarity, float64 [iou_size]."""
    _need_device("coco_oks", dt_kp, gt_kp, vars)
    for name, t in (("dt_kp", dt_kp), ("gt_kp", gt_kp), ("gt_boxes", gt_boxes), ("gt_area", gt_area), ("vars", vars)):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"coco_oks: {name} must be contiguous float64")
    K = int(vars.shape[0])
    nd, ngt = int(dt_kp.shape[0]), int(gt_kp.shape[0])
    if vars.dim() != 1 or tuple(dt_kp.shape) != (nd, K, 2) or tuple(gt_kp.shape) != (ngt, K, 3) or tuple(gt_boxes.shape) != (ngt, 4) \
            or tuple(gt_area.shape) != (ngt,):
        raise ValueError(f"coco_oks: with {K} vars, dt_kp must be [ND, {K}, 2], gt_kp [NG, {K}, 3], gt_boxes [NG, 4] and gt_area [NG]")
    out = torch.empty(int(iou_size), dtype=torch.float64, device=dt_kp.device)
    check(lib().mi355det_coco_oks(int(dt_offsets.shape[0]) - 1, ptr(dt_offsets), ptr(gt_offsets), ptr(iou_offsets), nd, ngt, int(iou_size), K,
                                  ptr(dt_kp), ptr(gt_kp), ptr(gt_boxes), ptr(gt_area), ptr(vars), ptr(out), stream_ptr()), "coco_oks")
    return out


def keypoints_match(dt_offsets, gt_offsets, iou_offsets, oks, dt_area, gt_area, gt_flag, gt_crowd, iou_thrs, area_rngs):
    """mi355det_keypoints_match (coco_match with the ignore flag gt_flag and the re-match flag gt_crowd apart, both uint8 [NG]) -> the four
    arrays of coco_match, same layouts."""
    _need_device("keypoints_match", oks)
    if gt_flag.dtype != torch.uint8 or gt_crowd.dtype != torch.uint8 or gt_flag.shape != gt_area.shape or gt_crowd.shape != gt_area.shape:
        raise ValueError("keypoints_match: gt_flag and gt_crowd must be uint8, one flag per ground truth")
    return _match(lib().mi355det_keypoints_match, "keypoints_match", dt_offsets, gt_offsets, iou_offsets, oks, dt_area, gt_area,
                  [gt_flag, gt_crowd], iou_thrs, area_rngs)


def coco_accumulate(cat_dt_offsets, cat_gt_offsets, order, dt_rank, dt_score, dt_match, dt_ignore, gt_ignore, max_dets, rec_thrs):
    """mi355det_coco_accumulate -> precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M] (float64)."""
    dev = rec_thrs.device
    _need_device("coco_accumulate", rec_thrs)
    K = int(cat_dt_offsets.shape[0]) - 1
    A, T, nd = (int(v) for v in dt_match.shape)
    ngt, R, M = int(gt_ignore.shape[1]), int(rec_thrs.shape[0]), len(max_dets)
    precision = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    recall = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    scores = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    md = (C.c_int32 * M)(*[int(m) for m in max_dets])
    check(lib().mi355det_coco_accumulate(K, ptr(cat_dt_offsets), ptr(cat_gt_offsets), nd, ngt, ptr(order), ptr(dt_rank), ptr(dt_score),
                                         ptr(dt_match), ptr(dt_ignore), ptr(gt_ignore), T, A, md, M, ptr(rec_thrs), R, ptr(precision),
                                         ptr(recall), ptr(scores), stream_ptr()), "coco_accumulate")
    return precision, recall, scores


def pooled_tile():
    """The number of list positions one wavefront of mi355det_pooled_accumulate owns per pass."""
    return int(lib().mi355det_pooled_tile())


def pooled_accumulate(pool_order, pool_offsets, pool_npig, dt_score, dt_match, dt_ignore, rec_thrs, pool_offsets_host=None):
    """mi355det_pooled_accumulate: pool_order int64 [P] (the pools' lists of detection slots, each in descending score order, concatenated),
    pool_offsets int64 [S + 1], pool_npig int64 [S, A], dt_score float64 [ND], dt_match int32 / dt_ignore uint8 [A, T, ND], rec_thrs
    float64 [R], all on the device -> precision [T, R, S, A], recall [T, S, A], scores [T, R, S, A] (float64).  `pool_offsets_host`: the
    caller's host copy of the offsets (a sequence of S + 1 ints); without it the offsets are read back here, the one host read."""
    import numpy as np
    what = "pooled_accumulate"
    _need_device(what, pool_order, pool_offsets, pool_npig, dt_score, dt_match, dt_ignore, rec_thrs)
    dev = rec_thrs.device
    for name, t, dt in (("pool_order", pool_order, torch.int64), ("pool_offsets", pool_offsets, torch.int64), ("pool_npig", pool_npig, torch.int64),
                        ("dt_score", dt_score, torch.float64), ("dt_match", dt_match, torch.int32), ("dt_ignore", dt_ignore, torch.uint8),
                        ("rec_thrs", rec_thrs, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous {dt}")
    S = int(pool_offsets.shape[0]) - 1
    A, T, nd = (int(v) for v in dt_match.shape)
    P, R = int(pool_order.shape[0]), int(rec_thrs.shape[0])
    if tuple(dt_ignore.shape) != (A, T, nd) or int(dt_score.shape[0]) != nd or tuple(pool_npig.shape) != (S, A):
        raise ValueError(f"{what}: dt_ignore must be [A, T, ND] like dt_match, dt_score [ND] and pool_npig [S, A]")
    host = np.ascontiguousarray(pool_offsets.cpu().numpy() if pool_offsets_host is None else pool_offsets_host, dtype=np.int64).reshape(-1)
    if host.shape[0] != S + 1:
        raise ValueError(f"{what}: the host copy of the offsets must hold S + 1 entries")
    precision = torch.empty((T, R, S, A), dtype=torch.float64, device=dev)
    recall = torch.empty((T, S, A), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, S, A), dtype=torch.float64, device=dev)
    nbytes = int(lib().mi355det_pooled_accumulate_workspace(P, S, T, A))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    check(lib().mi355det_pooled_accumulate(ptr(pool_order), P, ptr(pool_offsets), host.ctypes.data_as(C.c_void_p), S, ptr(pool_npig), nd,
                                           ptr(dt_score), ptr(dt_match), ptr(dt_ignore), T, A, ptr(rec_thrs), R, ptr(precision), ptr(recall),
                                           ptr(scores), ptr(ws), nbytes, stream_ptr()), what)
    return precision, recall, scores


def coco_bootstrap(cat_dt_offsets, cat_gt_offsets, order, dt_rank, dt_match, dt_ignore, gt_ignore, max_dets, rec_thrs, dt_image, gt_image,
                   weights):
    """mi355det_coco_bootstrap: coco_accumulate's operands without the scores, dt_image [ND] / gt_image [NG] int32 (each slot's image index)
    and weights int32 [num_images, B] (replicate-minor) -> ap_sum, recall float64 [B, T, K, A, M]."""
    _need_device("coco_bootstrap", weights, rec_thrs)
    dev = weights.device
    if weights.dtype != torch.int32 or weights.dim() != 2 or dt_image.dtype != torch.int32 or gt_image.dtype != torch.int32:
        raise ValueError("coco_bootstrap: weights [num_images, B], dt_image and gt_image must be int32")
    K = int(cat_dt_offsets.shape[0]) - 1
    A, T, nd = (int(v) for v in dt_match.shape)
    ngt, R, M = int(gt_ignore.shape[1]), int(rec_thrs.shape[0]), len(max_dets)
    I, B = (int(v) for v in weights.shape)
    if int(dt_image.shape[0]) != nd or int(gt_image.shape[0]) != ngt:
        raise ValueError("coco_bootstrap: one image index per detection slot and per ground truth")
    ap_sum = torch.full((B, T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    recall = torch.full((B, T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    md = (C.c_int32 * M)(*[int(m) for m in max_dets])
    w = weights.contiguous()
    check(lib().mi355det_coco_bootstrap(K, ptr(cat_dt_offsets), ptr(cat_gt_offsets), nd, ngt, ptr(order), ptr(dt_rank), ptr(dt_match),
                                        ptr(dt_ignore), ptr(gt_ignore), T, A, md, M, ptr(rec_thrs), R, ptr(dt_image), ptr(gt_image), ptr(w),
                                        I, B, ptr(ap_sum), ptr(recall), stream_ptr()), "coco_bootstrap")
    return ap_sum, recall


def _one_group(d, g, dev):
    off = lambda n: torch.tensor([0, n], dtype=torch.int64, device=dev)
    return off(d), off(g), off(d * g)


def coco_box_iou(dt_xywh, gt_xywh, iscrowd):
    """pycocotools maskUtils.iou on boxes: [D, 4] against [G, 4] as [x, y, w, h], iscrowd [G] -> float64 [D, G].  float32 inputs are widened
    exactly; all arithmetic is float64."""
    _need_device("coco_box_iou", dt_xywh)
    dev = dt_xywh.device
    dt, gt = _f64c(dt_xywh, dev).reshape(-1, 4), _f64c(gt_xywh, dev).reshape(-1, 4)
    crowd = torch.as_tensor(iscrowd, device=dev).to(torch.uint8).contiguous()
    D, G = int(dt.shape[0]), int(gt.shape[0])
    if crowd.shape[0] != G:
        raise ValueError("coco_box_iou: one iscrowd flag per ground truth")
    return coco_iou(*_one_group(D, G, dev), D * G, dt, gt, crowd).reshape(D, G)


def coco_mask_iou(dt, gt, iscrowd):
    """pycocotools maskUtils.iou on run-length encodings: RLEBatch [D] against RLEBatch [G] of the same [H, W] -> float64 [D, G]."""
    dev = dt.counts.device
    _need_device("coco_mask_iou", dt.counts)
    crowd = torch.as_tensor(iscrowd, device=dev).to(torch.uint8).contiguous()
    D, G = len(dt), len(gt)
    if crowd.shape[0] != G:
        raise ValueError("coco_mask_iou: one iscrowd flag per ground truth")
    side = lambda b: (b.counts.to(dev).contiguous(), torch.tensor(b.offsets, dtype=torch.int64, device=dev), None)
    rle = {"dt": side(dt), "gt": side(gt), "dt_sizes": [dt.size if D else (0, 0)], "gt_sizes": [gt.size if G else (0, 0)]}
    boxes = lambda b: b.stats()[1].to(dev).to(torch.float64).contiguous()
    return coco_iou(*_one_group(D, G, dev), D * G, boxes(dt), boxes(gt), crowd, rle).reshape(D, G)


def coco_boundary_iou(dt, gt, iscrowd, dilation_ratio=0.02):
    """The IoU that `iou_type="boundary"` matches on: min(mask IoU, boundary IoU), element by element, RLEBatch [D] against RLEBatch [G] of
    the same [H, W] -> float64 [D, G].  The boundary IoU is coco_mask_iou on RLEBatch.boundary(dilation_ratio) of both sides with the same
    iscrowd flags (a crowd ground truth divides by the detection's boundary area)."""
    _need_device("coco_boundary_iou", dt.counts, gt.counts)
    return torch.minimum(coco_mask_iou(dt, gt, iscrowd), coco_mask_iou(dt.boundary(dilation_ratio), gt.boundary(dilation_ratio), iscrowd))


# ---- model comparison (csrc/compare_kernels.hip; the front end on top of it is object_detectors_amd/compare.py)
def box_disagreement(gt_offsets, gt_box, gt_label, dt_a, dt_b, iou_threshold):
    """mi355det_box_disagreement: gt_offsets int64 [I + 1] (from 0 to G), gt_box float64 [G, 4] as [x, y, w, h], gt_label int64 [G]; dt_a / dt_b
    = (dt_offsets int64 [I + 1], dt_box float64 [D, 4], dt_label int64 [D]) of the two models, everything on the device ->
    best_iou float64 [2, G], best_index int32 [2, G] (within the image's detections; -1: the image has none), correct uint8 [2, G]."""
    tensors = (gt_offsets, gt_box, gt_label) + tuple(dt_a) + tuple(dt_b)
    _need_device("box_disagreement", *tensors)
    dev = gt_box.device
    i64c = lambda t: t.to(torch.int64).contiguous()
    I = int(gt_offsets.shape[0]) - 1
    gt_offsets, gt_box, gt_label = i64c(gt_offsets), _f64c(gt_box, dev).reshape(-1, 4), i64c(gt_label)
    G = int(gt_box.shape[0])
    if I < 0 or int(gt_label.shape[0]) != G:
        raise ValueError("box_disagreement: gt_offsets must hold I + 1 entries and every ground truth one label")
    sides = []
    for off, box, label in (dt_a, dt_b):
        off, box, label = i64c(off), _f64c(box, dev).reshape(-1, 4), i64c(label)
        if int(off.shape[0]) != I + 1 or int(label.shape[0]) != int(box.shape[0]):
            raise ValueError("box_disagreement: each model needs I + 1 offsets and one label per box")
        sides.append((off, box, label))
    best_iou = torch.empty((2, G), dtype=torch.float64, device=dev)
    best_index = torch.empty((2, G), dtype=torch.int32, device=dev)
    correct = torch.empty((2, G), dtype=torch.uint8, device=dev)
    args = [a for off, box, label in sides for a in (ptr(off), int(box.shape[0]), ptr(box), ptr(label))]
    check(lib().mi355det_box_disagreement(I, ptr(gt_offsets), G, ptr(gt_box), ptr(gt_label), *args, float(iou_threshold), ptr(best_iou),
                                          ptr(best_index), ptr(correct), stream_ptr()), "box_disagreement")
    return best_iou, best_index, correct


# ---- error breakdown (csrc/tide_kernels.hip; the front end on top of these is object_detectors_amd/tide.py)
def _tide_view(view, what):
    """(img_dt_offsets, img_dt_slots, img_gt_offsets, img_gt_slots), int64 on the device -> their pointers with the three sizes in place."""
    dt_off, dt_slots, gt_off, gt_slots = view
    for t in view:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()):
            raise ValueError(f"{what} needs the image view as contiguous int64 CUDA/HIP tensors (no CPU fallback)")
    I = int(dt_off.shape[0]) - 1
    if I < 0 or int(gt_off.shape[0]) != I + 1:
        raise ValueError(f"{what}: both offset tables must hold I + 1 entries")
    return I, (I, ptr(dt_off), ptr(dt_slots), int(dt_slots.shape[0]), ptr(gt_off), ptr(gt_slots), int(gt_slots.shape[0]))


def _tide_typed(what, n, **tensors):
    """Each named (tensor, dtype) must be a contiguous device tensor of that dtype with n leading entries."""
    for name, (t, dtype) in tensors.items():
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and int(t.shape[0]) == n):
            raise ValueError(f"{what}: {name} must be a contiguous {dtype} CUDA/HIP tensor with {n} entries")


def tide_classify(view, dt_boxes, dt_cat, dt_fp, gt_boxes, gt_cat, gt_counted, gt_free, fg=0.5, bg=0.1):
    """mi355det_tide_classify.  `view` = (img_dt_offsets [I + 1], img_dt_slots [ND], img_gt_offsets [I + 1], img_gt_slots [NG]) int64;
    boxes float64 [*, 4] as [x, y, w, h], dt_cat / gt_cat int32, dt_fp / gt_counted / gt_free uint8, all on the device ->
    kind uint8 [ND], partner int64 [ND], best_same / best_other float64 [ND], missed uint8 [NG]."""
    what = "tide_classify"
    _I, head = _tide_view(view, what)
    nd, ng, dev = head[3], head[6], view[0].device
    _tide_typed(what, nd, dt_boxes=(dt_boxes, torch.float64), dt_cat=(dt_cat, torch.int32), dt_fp=(dt_fp, torch.uint8))
    _tide_typed(what, ng, gt_boxes=(gt_boxes, torch.float64), gt_cat=(gt_cat, torch.int32), gt_counted=(gt_counted, torch.uint8),
                gt_free=(gt_free, torch.uint8))
    kind = torch.zeros(nd, dtype=torch.uint8, device=dev)
    partner = torch.full((nd,), -1, dtype=torch.int64, device=dev)
    best_same = torch.zeros(nd, dtype=torch.float64, device=dev)
    best_other = torch.zeros(nd, dtype=torch.float64, device=dev)
    missed = torch.zeros(ng, dtype=torch.uint8, device=dev)
    check(lib().mi355det_tide_classify(*head, ptr(dt_boxes), ptr(dt_cat), ptr(dt_fp), ptr(gt_boxes), ptr(gt_cat), ptr(gt_counted), ptr(gt_free),
                                       float(fg), float(bg), ptr(kind), ptr(partner), ptr(best_same), ptr(best_other), ptr(missed),
                                       stream_ptr()), what)
    return kind, partner, best_same, best_other, missed


def tide_fixes(view, dt_match, dt_ignore, dt_cat, gt_cat, gt_counted, gt_free, kind, partner, missed):
    """mi355det_tide_fixes.  `view` as in tide_classify; dt_match int32 [ND] / dt_ignore uint8 [ND] = the evaluator's rows at the analysis
    threshold, area `all`; kind / partner / missed from tide_classify -> fix_dt_match int32 [8, 1, ND], fix_dt_ignore uint8 [8, 1, ND],
    fix_gt_ignore uint8 [8, NG] (rows base, Loc, Both, Dupe, Bkg, Miss, FP, FN) and cls_cat int32, cls_match int32, cls_ignore uint8 [ND]."""
    what = "tide_fixes"
    _I, head = _tide_view(view, what)
    nd, ng, dev = head[3], head[6], view[0].device
    _tide_typed(what, nd, dt_match=(dt_match, torch.int32), dt_ignore=(dt_ignore, torch.uint8), dt_cat=(dt_cat, torch.int32),
                kind=(kind, torch.uint8), partner=(partner, torch.int64))
    _tide_typed(what, ng, gt_cat=(gt_cat, torch.int32), gt_counted=(gt_counted, torch.uint8), gt_free=(gt_free, torch.uint8),
                missed=(missed, torch.uint8))
    # a slot no image owns keeps the base state
    fix_dt_match = dt_match.reshape(1, 1, nd).repeat(8, 1, 1)
    fix_dt_ignore = dt_ignore.reshape(1, 1, nd).repeat(8, 1, 1)
    fix_gt_ignore = (gt_counted == 0).to(torch.uint8).reshape(1, ng).repeat(8, 1)
    cls_cat, cls_match, cls_ignore = dt_cat.clone(), dt_match.clone(), dt_ignore.clone()
    check(lib().mi355det_tide_fixes(*head, ptr(dt_match), ptr(dt_ignore), ptr(dt_cat), ptr(gt_cat), ptr(gt_counted), ptr(gt_free), ptr(kind),
                                    ptr(partner), ptr(missed), ptr(fix_dt_match), ptr(fix_dt_ignore), ptr(fix_gt_ignore), ptr(cls_cat),
                                    ptr(cls_match), ptr(cls_ignore), stream_ptr()), what)
    return fix_dt_match, fix_dt_ignore, fix_gt_ignore, cls_cat, cls_match, cls_ignore


# ---- weighted boxes fusion (csrc/fusion_kernels.hip; the front end on top of it is object_detectors_amd/ensemble.py)
WBF_CONF_TYPES = {"avg": 0, "max": 1}


def wbf_lds_clusters():
    """The number of a group's clusters whose fused boxes mi355det_wbf_fuse keeps in LDS; later clusters go through global memory."""
    return int(lib().mi355det_wbf_lds_clusters())


def wbf_fuse(group_offsets, boxes, scores, iou_thr=0.55, conf_type="avg", weight_sum=1.0, weight_max=1.0):
    """mi355det_wbf_fuse: group_offsets int64 [G + 1], boxes float64 [N, 4] as corners and scores float64 [N] (the weighted scores), both in
    fusion order, all on the device -> leader int64 [N] (the founder slot of each candidate's cluster; -1 for a slot no group owns), fused
    float64 [N, 4] (corners), score float64 [N], members int32 [N] and sums float64 [N, 6] (S1..S4, C, mx), the last four written at founder
    slots (leader[slot] == slot) only."""
    what = "wbf_fuse"
    _need_device(what, group_offsets, boxes, scores)
    if conf_type not in WBF_CONF_TYPES:
        raise ValueError(f"{what}: conf_type must be one of {sorted(WBF_CONF_TYPES)}, not {conf_type!r}")
    dev = boxes.device
    group_offsets = group_offsets.to(torch.int64).contiguous()
    boxes, scores = _f64c(boxes, dev).reshape(-1, 4), _f64c(scores, dev).reshape(-1)
    G, N = int(group_offsets.shape[0]) - 1, int(boxes.shape[0])
    if G < 0 or int(scores.shape[0]) != N:
        raise ValueError(f"{what}: group_offsets must hold G + 1 entries and every box one score")
    leader = torch.full((N,), -1, dtype=torch.int64, device=dev)
    founders = torch.empty(N, dtype=torch.int64, device=dev)
    sums = torch.empty((N, 6), dtype=torch.float64, device=dev)
    fused = torch.empty((N, 4), dtype=torch.float64, device=dev)
    score = torch.empty(N, dtype=torch.float64, device=dev)
    members = torch.empty(N, dtype=torch.int32, device=dev)
    check(lib().mi355det_wbf_fuse(ptr(group_offsets), G, N, ptr(boxes), ptr(scores), float(iou_thr), WBF_CONF_TYPES[conf_type], float(weight_sum),
                                  float(weight_max), ptr(leader), ptr(founders), ptr(sums), ptr(fused), ptr(score), ptr(members), stream_ptr()),
          what)
    return leader, fused, score, members, sums
