/* mi355det — C ABI of the MI355X-native detection hot path (libmi355det.so).
 *
 * Drop-in boundary for the one hot path of kostas1515/object_detectors.  The
 * reference has no FFI of its own: its boundary is a set of Python callables.  Each entry point
 * below names the reference callable (file:line under /root/reference) it replaces; the Python
 * mirror in object_detectors_amd/ binds them with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless it is
 *     marked "host".  The caller owns all buffers (inputs, outputs, workspace).
 *   - every call enqueues on `stream` (hipStream_t passed as void*) and returns immediately;
 *     no call synchronises, allocates or copies to the host.
 *   - return value: 0 = MI355DET_OK, negative = error (mi355det_last_error() gives the text);
 *     the library never throws and never aborts.
 *   - data-dependent output sizes (NMS keeps, compaction) are written to a caller-provided
 *     max-size buffer plus a device-side counter.
 *   - fp32 for boxes / losses / scores; bf16 (NHWC) for convolution activations and weights.
 */
#ifndef MI355DET_H
#define MI355DET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355DET_OK 0
#define MI355DET_EINVAL (-1)   /* bad argument / unsupported shape */
#define MI355DET_ELAUNCH (-2)  /* HIP launch failure */
#define MI355DET_EWORKSPACE (-3) /* workspace too small */

#define MI355DET_MAX_SCALES 4
#define MI355DET_MAX_ANCHORS 8

const char* mi355det_last_error(void);
int mi355det_debug_set(int key, int value);   /* bring-up / test knobs: key 0 = force a conv tile configuration (0 = tuned), 1 = weight gradient
                                                 with per-lane bookkeeping, 2 = stride-2 data gradient as four class launches (tests compare the forms),
                                                 3 = diagnostic build of the phase-staggered conv, 5 = stride-2 data-gradient form, 6 = weight-gradient
                                                 ablations (timing only), 7 = weight-gradient split count for every launch (+ 65536: the 256 x 256
                                                 phase-staggered kernel; fails for shapes it does not take), 8 = 1: the tuner leaves that kernel out,
                                                 9 = 1: strict mode - a configuration forced through key 0 that the launch would not run (predicate or
                                                 epilogue of the id fails, wide id on a narrow output or 29 / 30 / 31 on a wide one, unknown id, a route
                                                 without tile choice: single-launch stride 2, split-K conv_dgrad_ws, the fixed Cin % 64 != 0 tile) and a
                                                 split count forced through key 7 that is invalid for the pixel count or exceeds the workspace return
                                                 MI355DET_EINVAL and launch nothing; 0 (default) = they fall back silently (1 / the nearest valid split) */
int mi355det_debug_ptr(int key, void* ptr);   /* key 0 = device buffer for the diagnostic (phase-stamp) conv build */
int mi355det_version(void);

/* ------------------------------------------------------------------------------------------
 * YOLO criterion geometry (yolo/nets/yolo_forw.py:93-119).  Anchor index within an image is
 * off[k] + (y*W+x)*na + a, scales in the order the head returns them (stride 32, 16, 8).
 * anchor_w/h are the NORMALISED anchor sizes exactly as the reference computes them in float32:
 * float32(a_w / (img_size/grid)) / float32(grid).
 */
typedef struct {
  int32_t num_scales, na, num_classes, pad0;
  float img_size, ignore_thr;
  int32_t iou_type, pad1;                 /* 0 IoU, 1 GIoU, 2 DIoU, 3 CIoU (helper.py:224-231) */
  int32_t grid[MI355DET_MAX_SCALES];      /* H == W per scale */
  int32_t off[MI355DET_MAX_SCALES + 1];   /* prefix sums of grid^2*na; off[num_scales] == N */
  float anchor_w[MI355DET_MAX_SCALES][MI355DET_MAX_ANCHORS];
  float anchor_h[MI355DET_MAX_SCALES][MI355DET_MAX_ANCHORS];
} mi355det_yolo_geom;

/* A head tensor in place: element (b, a, attr, pix) at base + b*sb + (a*attrs+attr)*sc + pix*sp
 * (elements).  NCHW [bs,A*attrs,H,W]: sc=H*W, sp=1.  NHWC (engine native): sc=1, sp=row pitch. */
typedef struct {
  void* ptr;
  int64_t sb, sc, sp;
} mi355det_head_view;

typedef struct {
  float lambda_iou, lambda_xy, lambda_wh, lambda_conf, lambda_no_conf, lambda_cls;
  float alpha, gamma;          /* custom.FocalLoss (yolo/utilities/custom.py:40-67) */
  float grad_scale;            /* multiplies every gradient (1/sum(M) is applied internally) */
  int32_t grad_is_bf16;        /* format of the grad views: 0 = fp32, 1 = bf16 (engine default), 2 = IEEE fp16 (engine with fp16 storage) */
  const float* class_weights;  /* device [C] or NULL: nn.CrossEntropyLoss(weight=..., reduction='sum') class weights
                                  (yolo_forw.py:50-62,72: tf-idf / effective-number re-weighting); for class_loss 0 / 2 the same
                                  row is BCEWithLogitsLoss's pos_weight (yolo_forw.py:70-71,74-75) */
  int32_t class_loss;          /* cfg.class_loss (yolo_forw.py:69-77): 0 BCEWithLogitsLoss, 1 CrossEntropyLoss (the default), 2 custom.EQLoss */
  int32_t reduction_mean;      /* cfg.reduction: 0 'sum' (every term / sum(M), yolo_forw.py:158-160), 1 'mean' (each loss over its own
                                  element count, no final division) */
  const float* eq_mask;        /* device [C], class_loss 2 only: custom.EQLoss.eq_mask (custom.py:79-80, 1.0 where the class's image-frequency
                                  share is below 0.0045) */
} mi355det_yolo_loss_cfg;

/* helper.bbox_iou (yolo/utilities/helper.py:221-277), broadcast form [M,1,4] x [1,N,4] -> [M,N]
 * (elementwise form: M==1 rows paired, see `paired`).  xcycwh!=0 converts with get_abs_coord. */
int mi355det_bbox_iou(const float* bb1, const float* bb2, float* out, int64_t m, int64_t n,
                      int iou_type, int xcycwh, int paired, void* stream);

/* YOLOForw.get_target (yolo_forw.py:178-208), all images in one launch.
 *   gt_box [G,4] relative xcycwh, gt_off [bs+1] int32 prefix of per-image GT counts (device).
 * out: best_key [G] u64 scratch (zeroed by the call), obj_idx [G] int64, tgt [G,4],
 *      noobj [bs,N] uint8 (1 = contributes to the no-object loss). */
int mi355det_yolo_assign(const mi355det_yolo_geom* geom, const float* gt_box, const int32_t* gt_off,
                         int32_t bs, int32_t num_gt, int32_t max_gt_per_img, uint64_t* best_key,
                         int64_t* obj_idx, float* tgt, uint8_t* noobj, void* stream);

/* YOLOForw.forward, train branch (yolo_forw.py:121-162) fused forward+backward.
 *   heads/grads: num_scales views (grads may be NULL for forward only; grad buffers must be
 *   zero-filled by the caller — only conf planes and positive rows are written).
 *   gt_label [G] int64, idf [C] or NULL (idf_logits, yolo_forw.py:63-67,136).
 *   partials: float workspace of mi355det_yolo_loss_workspace(bs, N) bytes.
 *   out12: loss, sub_losses[6] (xy, wh, iou, pos_conf, neg_conf, cls; already / sum(M)), stats[5]. */
size_t mi355det_yolo_loss_workspace(int32_t bs, int64_t n_anchors);
int mi355det_yolo_loss(const mi355det_yolo_geom* geom, const mi355det_yolo_loss_cfg* cfg,
                       const mi355det_head_view* heads, const mi355det_head_view* grads,
                       const int32_t* gt_off, const int64_t* gt_label, const int64_t* obj_idx,
                       const float* tgt, const uint8_t* noobj, const float* idf, int32_t bs,
                       int32_t num_gt, void* workspace, size_t workspace_bytes, float* out12,
                       void* stream);

/* YOLOForw.forward, inference branch (yolo_forw.py:163-176): out [bs,N,attrs] fp32 contiguous.
 * softmax_cls!=0: class_loss is CrossEntropy (softmax), else sigmoid.
 * score_out/label_out [bs,N] (optional, channels-last heads only): conf*max(cls) and arg-max class
 * (test_one_epoch.py:25,35) produced in the same pass. */
int mi355det_yolo_decode(const mi355det_yolo_geom* geom, const mi355det_head_view* heads,
                         const float* idf, int32_t bs, int softmax_cls, float* out, float* score_out,
                         int32_t* label_out, void* stream);

/* test_one_epoch.py:24-35: get_abs_coord + score=conf*max(cls) + threshold + row build.
 * pred [bs,N,attrs] (decoded). cand [bs,max_cand,6] = (x1,y1,x2,y2,score,label), count [bs] int32
 * (true number of passing boxes, may exceed max_cand: caller must check).  Candidates keep the
 * anchor order of the reference's boolean mask. */
size_t mi355det_yolo_candidates_workspace(int32_t bs, int64_t n);
int mi355det_yolo_candidates(const float* pred, const float* score_in /* optional: from yolo_decode */,
                             const int32_t* label_in, int32_t bs, int64_t n, int32_t attrs, float conf_thr,
                             float* cand, int32_t* count, int32_t max_cand, void* workspace,
                             size_t workspace_bytes, void* stream);

/* helper.nms_majority (helper.py:280-382), batched over images.
 *   boxes [bs,max_n,6], count [bs] int32 (device).  Equal scores are ordered "stable ascending
 *   argsort" (highest original index first among ties).
 * out: out_rows [bs,max_n,6] kept rows in keep order with the majority relabel applied,
 *      out_idx [bs,max_n] int32 original row index, out_count [bs] int32.
 * max_n <= 131072 (up to 16384 boxes are sorted by one workgroup in LDS, more by chunk sorts + a merge by rank; the n*n/8-byte
 * suppression mask is 2 GiB per image at the cap).  workspace: mi355det_nms_workspace(bs, max_n). */
size_t mi355det_nms_workspace(int32_t bs, int32_t max_n);
int mi355det_nms_majority(const float* boxes, const int32_t* count, int32_t bs, int32_t max_n,
                          float thresh_iou, int32_t num_classes /* labels in [0,num_classes) */, float* out_rows, int32_t* out_idx, int32_t* out_count,
                          void* workspace, size_t workspace_bytes, void* stream);

/* torchvision.ops.boxes.box_iou (call sites: tvision/retinanet.py:409, rpn.py:192, roi_heads.py:633) */
int mi355det_box_iou(const float* boxes1, const float* boxes2, float* out, int64_t m, int64_t n,
                     void* stream);

/* torchvision.ops.boxes.nms / batched_nms (retinanet.py:463, rpn.py:272, roi_heads.py:771).
 *   boxes [n,4] xyxy, scores [n], idxs [n] int64 or NULL (plain nms); n <= 131072.
 *   keep [n] int64 in descending-score order (ties: lower index first), keep_count [1] int32. */
int mi355det_nms(const float* boxes, const float* scores, const int64_t* idxs, int32_t n,
                 float iou_thr, int64_t* keep, int32_t* keep_count, void* workspace,
                 size_t workspace_bytes, void* stream);

/* The same NMS for `bs` independent box sets of `n` boxes each in ONE launch sequence (replaces the per-image loop around
 * box_ops.batched_nms in RegionProposalNetwork.filter_proposals, tvision/rpn.py:259-280): boxes [bs,n,4], scores [bs,n], idxs [bs,n] or
 * NULL, keep [bs,n] (the first keep_count[b] entries of row b are defined), keep_count [bs].  Workspace: mi355det_nms_workspace(bs, n). */
int mi355det_nms_batch(const float* boxes, const float* scores, const int64_t* idxs, int32_t bs, int32_t n, float iou_thr, int64_t* keep,
                       int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream);

/* RegionProposalNetwork.filter_proposals for the whole batch in one call (tvision/rpn.py:215-280, with the anchor decode of :336-351
 * restricted to the selected anchors): per-level top-k of the objectness logits, decode (BoxCoder weights 1, clamp xform_clip), clip to
 * clip_limits[img] = (w, h, w, h), boxes smaller than min_size or scoring below score_thresh masked out, per-level NMS, the first
 * post_nms_top_n survivors of every image.  objectness [N, A] fp32 logits and deltas [N, A, 4], A = sum(level_counts) with the levels
 * concatenated in pyramid order; anchors [A, 4] xyxy; level_counts [nlev] on the HOST (nlev <= 8).  Outputs: out_boxes [N, post, 4],
 * out_scores [N, post] (sigmoid), out_counts [N] int32 on the device - rows beyond out_counts[img] are zero.  Results are those of
 * mi355det_topk + mi355det_box_decode + the clip / mask chain + mi355det_nms_batch, bit for bit.
 * Workspace: mi355det_rpn_proposals_workspace (0 for invalid arguments). */
size_t mi355det_rpn_proposals_workspace(int32_t n_images, const int64_t* level_counts, int32_t nlev, int32_t pre_nms_top_n);
int mi355det_rpn_proposals(const float* objectness, const float* deltas, const float* anchors, const float* clip_limits, int32_t n_images,
                           const int64_t* level_counts, int32_t nlev, int32_t pre_nms_top_n, int32_t post_nms_top_n, float nms_thresh,
                           float score_thresh, float min_size, float xform_clip, float* out_boxes, float* out_scores, int32_t* out_counts,
                           void* workspace, size_t workspace_bytes, void* stream);

/* RetinaNet.postprocess_detections for the whole batch in one call (tvision/retinanet.py:414-472): per level the scores above the threshold
 * (logit_thresh = logit of score_thresh: sigmoid is monotone), of those the topk_candidates best of the flattened [HWA_l x K] scores of
 * every image, decode of their anchors (BoxCoder weights 1), clip to clip_limits[img] = (w, h, w, h), per-class NMS, the first
 * detections_per_img survivors.  HOST tables per level: cls_logits[l] [N, HWA_l, K] fp32 (already scaled by the tf-idf row if any),
 * bbox_regression[l] [N, HWA_l, 4], anchors[l] [HWA_l, 4], level_anchors[l] = HWA_l.  Outputs: out_boxes [N, det, 4], out_scores [N, det],
 * out_labels [N, det] int64, out_counts [N] int32 on the device; rows beyond out_counts[img] are zero.  The same results as
 * mi355det_topk_ws + mi355det_box_decode + clip + mi355det_nms_batch.  Workspace: mi355det_retina_detections_workspace (0 = bad arguments). */
size_t mi355det_retina_detections_workspace(int32_t n_images, const int64_t* level_anchors, int32_t nlev, int32_t num_classes, int32_t topk_candidates);
int mi355det_retina_detections(const float* const* cls_logits, const float* const* bbox_regression, const float* const* anchors,
                               const int64_t* level_anchors, int32_t nlev, int32_t n_images, int32_t num_classes, const float* clip_limits,
                               float logit_thresh, int32_t topk_candidates, float nms_thresh, int32_t detections_per_img, float xform_clip,
                               float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* out_counts, void* workspace,
                               size_t workspace_bytes, void* stream);

/* RoIHeads.postprocess_detections for the whole batch in one call (tvision/roi_heads.py:715-781): scores [N, P, C] (the reference's score
 * function already applied; the caller pushes class 0 and padded proposals below score_thresh), box_regression [N, P, C, 4], proposals
 * [N, P, 4], clip_limits [N, 4] = (w, h, w, h).  Candidates = the scores above score_thresh, at most max_candidates per image in descending
 * order (candidate_counts[img] == max_candidates means the list may be truncated: the caller then takes the unbounded route); decode with
 * BoxCoder(wx, wy, ww, wh), clip, boxes smaller than min_size masked, per-class NMS, the first detections_per_img survivors ->
 * out_boxes [N, det, 4], out_scores [N, det], out_labels [N, det] int64, out_counts [N], candidate_counts [N] (int32, device). */
size_t mi355det_roi_detections_workspace(int32_t n_images, int32_t max_proposals, int32_t num_classes, int32_t max_candidates);
int mi355det_roi_detections(const float* scores, const float* box_regression, const float* proposals, const float* clip_limits, int32_t n_images,
                            int32_t max_proposals, int32_t num_classes, float score_thresh, int32_t max_candidates, float wx, float wy, float ww,
                            float wh, float xform_clip, float min_size, float nms_thresh, int32_t detections_per_img, float* out_boxes,
                            float* out_scores, int64_t* out_labels, int32_t* out_counts, int32_t* candidate_counts, void* workspace,
                            size_t workspace_bytes, void* stream);

/* RegionProposalNetwork.compute_loss (tvision/rpn.py:282-318) on prepared indices, forward and gradient in one launch: objectness [T] logits,
 * pred_bbox_deltas / regression_targets [T,4], labels [T] (1 / 0 for the sampled anchors), pos_idx [num_pos] and sampled_idx [num_sampled]
 * (positives followed by negatives, unique).  losses[0] = binary_cross_entropy_with_logits(objectness[sampled], labels[sampled]) (mean),
 * losses[1] = smooth_l1(deltas[pos], targets[pos], beta 1/9, sum) / num_sampled; grad_objectness [T] and grad_deltas [T,4] are their
 * gradients (zero outside the sampled / positive anchors), written completely. */
int mi355det_rpn_loss(const float* objectness, const float* pred_bbox_deltas, const float* labels, const float* regression_targets, int64_t total,
                      const int64_t* pos_idx, int32_t num_pos, const int64_t* sampled_idx, int32_t num_sampled, float* losses, float* grad_objectness,
                      float* grad_deltas, void* stream);

/* RoIHeads.select_training_samples for the whole batch (tvision/roi_heads.py:627-713), the two launches around the one host read its
 * sampler needs.  Candidates of image i are its proposals (proposals [N, max_proposals, 4] padded, proposal_counts [N] on the device, as
 * mi355det_rpn_proposals leaves them) followed by its ground truth (add_gt_proposals): gt_boxes [G,4] / gt_labels [G] of all images
 * concatenated, gt_offsets [N+1] on the HOST (1..1024 boxes per image; at most 64 images, 8192 candidates per image).
 *   mi355det_roi_match: box_iou + Matcher(fg_iou_thresh, bg_iou_thresh, no low-quality rescue) + assign_targets_to_proposals ->
 *     matched [N, row_stride] (clamped at 0), labels [N, row_stride] (-1 between the thresholds, 0 background, else the class),
 *     counts [N, 2] = positives (label >= 1), negatives (label == 0).
 *   mi355det_roi_sample: perm_pos[i] / perm_neg[i] (HOST tables of device pointers) are `torch.randperm(positives_i)` /
 *     `randperm(negatives_i)`, of which the first num_pos[i] / num_neg[i] (HOST) are used exactly as BalancedPositiveNegativeSampler
 *     does (tvision/_utils.py:38-73); outputs for the sum(num_pos + num_neg) samples in image order, ascending candidate index inside an
 *     image: rois [S, 5] = (image, box), out_labels [S], out_matched [S], out_regression_targets [S, 4] = BoxCoder(wx, wy, ww, wh).encode. */
int mi355det_roi_match(const float* proposals, const int32_t* proposal_counts, int32_t n_images, int32_t max_proposals, const float* gt_boxes,
                       const int64_t* gt_labels, const int32_t* gt_offsets, float fg_iou_thresh, float bg_iou_thresh, int32_t row_stride,
                       int32_t* matched, int32_t* labels, int32_t* counts, void* stream);
int mi355det_roi_sample(const float* proposals, const int32_t* proposal_counts, int32_t n_images, int32_t max_proposals, const float* gt_boxes,
                        const int32_t* gt_offsets, int32_t row_stride, const int32_t* matched, const int32_t* labels,
                        const int64_t* const* perm_pos, const int64_t* const* perm_neg, const int32_t* num_pos, const int32_t* num_neg, float wx,
                        float wy, float ww, float wh, float* rois, int64_t* out_labels, int64_t* out_matched, float* out_regression_targets,
                        void* stream);

/* box_iou + Matcher.__call__ (+ set_low_quality_matches_) fused, never materialising [M,N]
 * (tvision/_utils.py:271-344 after retinanet.py:409).  gt [M,4], anchors [N,4] xyxy.
 * out matches [N] int64 in {-2,-1,0..M-1}; gt_best [M] uint32 scratch. */
int mi355det_match_anchors(const float* gt, const float* anchors, int32_t m, int64_t n, float high_thr,
                           float low_thr, int allow_low_quality, uint32_t* gt_best, int64_t* matches,
                           void* stream);

/* BoxCoder.encode_single / decode_single (tvision/_utils.py:79-125,190-223).  decode: codes [n,4*k] */
int mi355det_box_encode(const float* reference_boxes, const float* proposals, float* out, int64_t n,
                        float wx, float wy, float ww, float wh, void* stream);
int mi355det_box_decode(const float* codes, const float* boxes, float* out, int64_t n, int32_t k,
                        float wx, float wy, float ww, float wh, float clip, void* stream);

/* AnchorGenerator.grid_anchors for one level (tvision/anchor_utils.py:98-134):
 * out [gh*gw*a,4] = shifts(y outer, x inner) + cell[a] ; cell [a,4] from the host (rounded). */
int mi355det_anchor_grid(const float* cell, int32_t a, int32_t gh, int32_t gw, int32_t stride_h,
                         int32_t stride_w, float* out, void* stream);

/* torchvision.ops.sigmoid_focal_loss (retinanet.py:137-141) fused forward (+sum) and backward.
 *   x,t [n] ; scale [k] or NULL multiplies logits per class column (tfidf, retinanet.py:138) with
 *   n = rows*k; valid [rows] uint8 or NULL row mask; loss_sum [1] (atomically accumulated, caller
 *   zeroes), grad [n] or NULL = d(sum)/dx * grad_scale. */
int mi355det_sigmoid_focal_loss(const float* x, const float* t, const float* scale, const uint8_t* valid,
                                int64_t rows, int32_t k, float alpha, float gamma, float grad_scale,
                                float* loss_sum, float* grad, void* stream);
/* reduction = 'none' - torchvision's DEFAULT (the reference only calls 'sum': tvision/retinanet.py:137-141, roi_heads.py:57-58): the
 * unreduced loss per element and, if grad != NULL, d loss / d x per element; x, t, loss, grad are n contiguous floats. */
int mi355det_sigmoid_focal_loss_elem(const float* x, const float* t, int64_t n, float alpha, float gamma, float* loss,
                                     float* grad, void* stream);

/* RetinaNet classification loss without the dense one-hot target (retinanet.py:107-143):
 *   logits [rows,k], matched [rows] int64 (Matcher output), gt_labels [M] int64. Same outputs. */
int mi355det_retina_cls_loss(const float* logits, const int64_t* matched, const int64_t* gt_labels,
                             const float* scale, int64_t rows, int32_t k, float alpha, float gamma,
                             float grad_scale, float* loss_sum, float* grad, void* stream);

/* RetinaNetHead.compute_loss for a WHOLE batch in three launches (retinanet.py:56-62,107-143,196-223):
 *   cls_logits [n_images, rows_per_image, k], bbox_regression [n_images, rows_per_image, 4] (the level-concatenated head
 *   outputs), anchors [rows_per_image, 4] (same image size for the batch), matched [n_images, rows_per_image] int64
 *   (Matcher output: >=0 GT index within the image, -1 background, -2 between thresholds), gt_boxes [sum M,4] /
 *   gt_labels [sum M] packed over images with gt_offsets [n_images+1].
 *   losses[0] = classification (focal sum / max(1,num_fg) averaged over images), losses[1] = bbox_regression (L1 on
 *   BoxCoder(1,1,1,1) targets, same normalisation); num_fg [n_images] scratch/out; grads (nullable) = d(loss)*grad_scale. */
int mi355det_retina_loss(const float* cls_logits, const float* bbox_regression, const float* anchors, const int64_t* matched,
                         const float* gt_boxes, const int64_t* gt_labels, const int32_t* gt_offsets,
                         const float* class_scale, int32_t n_images, int64_t rows_per_image, int32_t k, float alpha,
                         float gamma, float grad_scale, float* num_fg, float* losses, float* grad_logits,
                         float* grad_regression, void* stream);

/* The same head loss with the classification gradient written where the head's backward reads it (replaces the autograd hand-over between
 * retinanet.py:107-143 and the cls_logits convolution, retinanet.py:75-105): bf16, per pyramid level an NHWC buffer [n_images, pixels, ld]
 * whose channel a*k + c is anchor a, class c of the pixel (exactly the layout of the level-concatenated logits [n, sum HWA, k]).  Saves the
 * fp32 gradient tensor and its cast (2 x 4 B per logit: 9 GB per step for the 1204-class head at batch 8).  Padding channels of the
 * buffers are not written (zero them once).  sum(pixels[q]) * anchors_per_pixel must equal rows_per_image. */
typedef struct {
  int32_t n_levels;             /* 1..8 */
  int32_t anchors_per_pixel;
  int64_t pixels[8];            /* h*w of each level */
  void* grad[8];                /* bf16 [n_images, pixels, grad_ld] */
  int32_t grad_ld[8];           /* >= anchors_per_pixel * k */
} mi355det_level_grads;
int mi355det_retina_loss_lv(const float* cls_logits, const float* bbox_regression, const float* anchors, const int64_t* matched,
                            const float* gt_boxes, const int64_t* gt_labels, const int32_t* gt_offsets, const float* class_scale,
                            int32_t n_images, int64_t rows_per_image, int32_t k, float alpha, float gamma, float grad_scale,
                            float* num_fg, float* losses, const mi355det_level_grads* cls_levels, float* grad_regression, void* stream);

/* torchvision.ops.roi_align / MultiScaleRoIAlign (tvision/frcnn.py:208-211, roi_heads.py:818): NCHW fp32 features.
 *   feats/hs/ws/scales: HOST arrays of num_levels (1..4) device pointers / sizes / spatial scales; with several levels
 *   the LevelMapper (k = floor(4 + log2(sqrt(area)/224) + 1e-6) clamped to [k_min,k_max]) picks the level per RoI.
 *   rois [K,5] = (batch index, x1,y1,x2,y2).  Forward: out [K,C,ph,pw].  Backward (grad_out != NULL): scatters
 *   grad_out into grad_feats (fp32 atomics, caller zeroes), `out` unused. */
int mi355det_roi_align(const float* const* feats, const int32_t* hs, const int32_t* ws, const float* scales,
                       int32_t num_levels, const float* rois, int32_t num_rois, int32_t channels,
                       int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio, int aligned, int32_t k_min,
                       int32_t k_max, float* out, const float* grad_out, float* const* grad_feats, void* stream);

/* Channels-last form of the same op for the engines' native layout: feats = bf16 NHWC [n,h,w,C] with pixel pitch lds[q]
 * (NULL = C); out / grad_out stay [K,C,ph,pw] fp32 (the order box_head.fc6 consumes, frcnn.py:248-262); grad_feats = dense
 * fp32 NHWC [n,h,w,C] buffers, zeroed by the caller.  Lanes run over channels, so the backward's atomics are contiguous
 * 256-byte runs instead of 64 scattered rows. */
int mi355det_roi_align_nhwc(const void* const* feats, const int32_t* hs, const int32_t* ws, const int32_t* lds,
                            const float* scales, int32_t num_levels, const float* rois, int32_t num_rois,
                            int32_t channels, int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio, int aligned,
                            int32_t k_min, int32_t k_max, float* out, const float* grad_out, float* const* grad_feats,
                            void* stream);

/* Tensor.topk(k, dim=1) on [rows, n] (tvision/rpn.py:215-228, retinanet.py:437-445): indices (and values) of the k
 * largest entries per row in descending order, ties -> lower index; entries <= min_value are never selected
 * (the "> score_thresh" filter).  idx_out/val_out [rows,k], count_out [rows] = number selected; k <= 16384. */
int mi355det_topk(const float* x, int32_t rows, int64_t n, int64_t row_stride, int32_t k, float min_value,
                  int64_t* idx_out, float* val_out, int32_t* count_out, void* stream);
/* the same for LONG rows (n >= 65536: several workgroups per row, 3 histogram launches + collect + sort); shorter rows are forwarded to
 * mi355det_topk.  workspace: mi355det_topk_workspace(rows) bytes. */
size_t mi355det_topk_workspace(int32_t rows);
int mi355det_topk_ws(const float* x, int32_t rows, int64_t n, int64_t row_stride, int32_t k, float min_value, int64_t* idx_out,
                     float* val_out, int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same selection for rows cut into up to 8 SEGMENTS (the pyramid levels of RegionProposalNetwork._get_top_n_idx, tvision/rpn.py:215-228):
 * segment s of row r is x[r*row_stride + seg_start[s] ...][0..seg_n[s]), its k = seg_k[s] <= seg_n[s]; outputs per segment idx_out[s]
 * [rows, k] (index WITHIN the segment), val_out[s] [rows, k] (val_out or its entries may be NULL), count_out[s] [rows].  Segments shorter
 * than 65536 share ONE launch (a workgroup per row and segment), longer ones take the mi355det_topk_ws route.  seg_* and the pointer
 * tables are HOST arrays.  workspace: mi355det_topk_workspace(rows) bytes. */
int mi355det_topk_segments(const float* x, int32_t rows, int64_t row_stride, int32_t nseg, const int64_t* seg_start, const int64_t* seg_n,
                           const int32_t* seg_k, float min_value, int64_t* const* idx_out, float* const* val_out, int32_t* const* count_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution path (yolo/nets/backbone/darknet.py:13-20,41-43,64-66; yolo/nets/yolohead.py:41-61):
 * NHWC bf16 activations, fp32 accumulation on MFMA.  See conv section in DESIGN.md.
 */
typedef struct {
  int32_t n, h, w, cin;        /* input  [n,h,w,cin], pixel pitch in_ld elements */
  int32_t ho, wo, cout;        /* output [n,ho,wo,cout], pixel pitch out_ld */
  int32_t ksize, stride, pad;  /* 1 or 3; 1 or 2; (k-1)/2 */
  int32_t in_ld, out_ld;
} mi355det_conv_shape;

/* Forward implicit GEMM: y = conv(x, w) [+ bias]; w packed [cout_pad][k*k*cin] bf16 (K contiguous).
 *   out_f32 != 0: y is fp32 (head conv_out), else bf16 (cout % 8 == 0: stored in 8-channel pieces).  Only the cout real channels of
 *   each pixel are written; pitch padding of x, y and the residual is never read or written.
 *   stats != NULL: per pixel-tile partial sums / sums of squares of y, stats[row][0][c], stats[row][1][c]
 *   (fp32, row pitch 2*cout_pad, plain stores, deterministic) for training BatchNorm. */
int mi355det_conv_fwd(const mi355det_conv_shape* s, const void* x, const void* w, const float* bias,
                      void* y, int out_f32, float* stats, int32_t cout_pad, void* stream);
/* Forward with a fused affine epilogue: y = relu?( conv(x,w) * scale[co] + shift[co] + residual ) — FrozenBatchNorm2d
 * (+ReLU, + the Bottleneck identity add, utilities/resnet.py:116-141) or a plain bias (FPN / RetinaNet head convs,
 * retinanet.py:86-97) without a separate elementwise pass. */
typedef struct {
  const float* scale;        /* [cout] or NULL (= 1) */
  const float* shift;        /* [cout] or NULL (= 0) */
  const void* residual;      /* bf16 [n,ho,wo,cout] with pixel pitch residual_ld, or NULL; bf16 outputs only */
  int32_t residual_ld;
  int32_t relu;              /* 0: none; 1: ReLU after scale/shift/residual (ResNet); 2: LeakyReLU(slope) after scale/shift and
                                BEFORE the residual (Darknet residual block, darknet.py:23-35) */
  int64_t out_image_stride;  /* fp32 outputs: elements between images of y (0 = ho*wo*out_ld): heads write straight
                                into the level-concatenated [N, sum HWA, K] tensor (retinanet.py:163-170) */
  float slope;               /* relu == 2: negative slope */
} mi355det_conv_epilogue;
int mi355det_conv_fwd_ex(const mi355det_conv_shape* s, const void* x, const void* w, const mi355det_conv_epilogue* e,
                         void* y, int out_f32, int32_t cout_pad, void* stream);
/* plan-build helper (synchronises; never part of the step): while the mode is on, mi355det_conv_fwd / _dgrad time
 * their candidate tile configurations on the caller's buffers and remember the fastest per shape. */
int mi355det_conv_autotune_mode(int on);

/* ---- tune record.  The plan build of both engines (yolo/nets/engine.py:_autotune, tvision/engine.py:_autotune; reference: none - the
 * reference lets cuDNN pick its algorithms per process, torch.backends.cudnn.benchmark, yolo/main.py) chooses by TIMING: the tile configuration
 * of every implicit-GEMM shape, the form of the stride-2 data gradient, the split count of every weight gradient.  Each choice fixes a
 * summation order, so the numbers of a step depend on it.  The record makes the choices data:
 *   export   copies the current choices as 16-byte entries sorted by (table, key) into buf (if cap suffices); returns the bytes needed
 *   import   adds (replace = 0) or replaces (1) the choices from a record
 *   lock     on = 1: a shape that HAS an entry is never timed again (plan builds reuse the record; shapes without an entry are timed and
 *            added as before); returns the previous state
 *   clear    drops every choice and the lock (the next plan build times everything)
 * Host mirror: object_detectors_amd/tune.py (JSON files, MI355DET_TUNE_SAVE / MI355DET_TUNE_LOAD, rank-0 broadcast for N > 1). */
typedef struct {
  uint32_t table;   /* 0 implicit-GEMM tile configuration, 1 stride-2 data-gradient form, 2 weight-gradient split count (+ 65536: the 256 x 256
                       phase-staggered kernel; a shape it does not take falls back to the 128 x 128 kernel with the same split count) */
  int32_t value;
  uint64_t key;     /* shape key of that table */
} mi355det_tune_entry;
size_t mi355det_tune_export(void* buf, size_t cap);
int mi355det_tune_import(const void* buf, size_t bytes, int replace);
int mi355det_tune_lock(int on);
int mi355det_tune_clear(void);
/* number of rows of the `stats` partial buffer [rows][2][cout_pad] the forward writes (one per pixel tile);
 * allocate rows+64: bn_finalize uses the 64 spare rows as scratch for its two-stage reduction */
int mi355det_conv_stats_rows(const mi355det_conv_shape* s, int32_t cout_pad);
/* Darknet stem (darknet.py:41, 3->32 3x3): NCHW fp32 image -> im2col rows [n*h*w][32] bf16
 * (k=(kh*3+kw)*3+c, 27 valid) consumed by conv_fwd / conv_wgrad as a 1x1 convolution with cin=32. */
int mi355det_stem_im2col(const float* img, void* out, int32_t n, int32_t h, int32_t w, void* stream);

/* Darknet stem without a stored pre-BN tensor (darknet.py:41-43,74-76: conv1 -> bn1 -> LeakyReLU; csrc/stem_kernels.hip).  The 3->32 3x3
 * convolution is recomputed from the fp32 NCHW image in every pass (K = 27: cheaper than one pass over the 32-channel tensor), so the
 * step never writes z, the im2col matrix or dz of this layer.  w = packed forward weights [32][32] bf16, k = (kh*3+kw)*3 + c
 * (mi355det_pack_weights of the [32, 32] "1x1" master the engine keeps).  Needs h % 8 == 0 and w % 32 == 0 (MI355DET_EINVAL otherwise).
 *   stem_rows            number of partial rows the kernels write (one per persistent workgroup); allocate rows + 64 for
 *                        bn_finalize / bn_bwd_sum_partials, rows * 1024 floats for the wgrad slab
 *   stem_fwd_stats       partial[rows][2][32]: per-channel sum z, sum z*z (fp32 z)            -> mi355det_bn_finalize
 *   stem_fwd_apply       a = lrelu(z*scale + shift) as bf16 NHWC (pitch a_ld); training AND eval (scale_shift from
 *                        mi355det_bn_finalize or mi355det_bn_eval_scale_shift)
 *   stem_bwd_reduce      partial[rows][2][32]: sum dy, sum dy*xhat, dy = da * lrelu'(z*scale+shift) -> mi355det_bn_bwd_sum_partials
 *   stem_bwd_apply_wgrad dz = scale*(dy - mean dy - xhat*mean(dy*xhat)) feeds the weight-gradient MFMA directly:
 *                        dw[32][32] += dz^T * im2col (fixed order via slab[rows][1024]); dgamma += sums[32..63], dbeta += sums[0..31]
 * All four are fixed-order (bit-reproducible). */
/* Stem activation + the first down-sampling convolution fused (csrc/stem_l1_kernels.hip; darknet.py:41-43,64-66,74-76): per 8 x 16 tile of
 * z1 = layer1.ds_conv(a0) the kernel recomputes a0 = lrelu(bn1(conv1(img))) (scale_shift0 from mi355det_bn_finalize of stem_fwd_stats) into
 * LDS and convolves it there (32 -> 64, 3x3, stride 2, pad 1; w1 = that layer's forward pack [64][9*32]).  Writes z1 (bf16 NHWC, pitch
 * z1_ld >= 64), its BatchNorm partial statistics stats[rows + 64][2][64] (rows = mi355det_stem_l1_rows) and - when a0 != NULL - the
 * activation itself (pitch a0_ld >= 32) for the layer's weight gradient.  Replaces stem_fwd_apply + conv_fwd of that layer in training.
 * Needs h % 16 == 0 and w % 32 == 0. */
int mi355det_stem_l1_rows(int32_t n, int32_t h, int32_t w);
int mi355det_stem_l1_fwd(const float* img, const void* w0, const float* scale_shift0, float slope, const void* w1, void* a0,
                         int32_t a0_ld, void* z1, int32_t z1_ld, float* stats, int32_t n, int32_t h, int32_t w, void* stream);
/* Inference form of the same launch: stem activation (folded BN: scale_shift0 from mi355det_bn_eval_scale_shift) + layer1.ds_conv + ITS folded
 * BN + LeakyReLU; a1 [n, h/2, w/2, 64] bf16 is the layer's ACTIVATION, the stem activation is never stored (839 MB written and read back at
 * batch 32 / 640 px otherwise).  scale_shift1 = scale[64] | shift[64] of layer 1. */
int mi355det_stem_l1_fwd_eval(const float* img, const void* w0, const float* scale_shift0, float slope, const void* w1,
                              const float* scale_shift1, void* a1, int32_t a1_ld, int32_t n, int32_t h, int32_t w, void* stream);
int mi355det_stem_rows(int32_t n, int32_t h, int32_t w);
int mi355det_stem_fwd_stats(const float* img, const void* w, float* partial, int32_t n, int32_t h, int32_t wd, void* stream);
int mi355det_stem_fwd_apply(const float* img, const void* w, const float* scale_shift, float slope, void* a, int32_t a_ld,
                            int32_t n, int32_t h, int32_t wd, void* stream);
int mi355det_stem_bwd_reduce(const float* img, const void* w, const float* scale_shift, float slope, const void* da,
                             int32_t da_ld, float* partial, int32_t n, int32_t h, int32_t wd, void* stream);
int mi355det_stem_bwd_apply_wgrad(const float* img, const void* w, const float* scale_shift, const float* sums, float slope,
                                  const void* da, int32_t da_ld, float* slab, float* dw, float* dgamma, float* dbeta,
                                  int32_t n, int32_t h, int32_t wd, void* stream);

/* The stem's backward in ONE pass over the activation gradient instead of stem_bwd_reduce + stem_bwd_apply_wgrad (same reference lines:
 * the autograd of darknet.py:41-43,74-76).  stem_bwd_fused accumulates, on MFMA over the pixels, A[32][32] = dy^T [im2col | 1] and the Gram
 * matrix G[32][32] = [im2col | 1]^T [im2col | 1] into slab[rows][2][32][32] (rows = mi355det_stem_rows), folds them into ag[2][32][32] and
 * derives sums[64] = (sum dy, sum dy*xhat) from A (sum dy = A[:,27], sum dy*z = <W, A>).  stem_bwd_finish then forms, from ag and the -
 * possibly rank-averaged, SyncBN - sums, dW += scale*(A - mean(dy)*B - mean(dy*xhat)*invstd*(W G - mean*B)) with B = G[27,:], and adds
 * dgamma += sums[32:], dbeta += sums[:32] (both nullable together).  count = n*h*w of THIS rank.  dw is [32][32] fp32 (k padded). */
int mi355det_stem_bwd_fused(const float* img, const void* w, const float* scale_shift, float slope, const void* da, int32_t da_ld,
                            float* slab, float* ag, float* sums, int32_t n, int32_t h, int32_t wd, void* stream);
int mi355det_stem_bwd_finish(const void* w, const float* scale_shift, const float* ag, const float* sums, int64_t count, float* dw,
                             float* dgamma, float* dbeta, void* stream);

/* Data gradient: dx = conv_transpose(dy, w); wt packed for dgrad by mi355det_pack_weights.  cin % 8 == 0.
 * residual != NULL adds a bf16 tensor (same shape as dx) in the epilogue (residual-block skip).  Rounding of the residual form, per route:
 *   implicit-GEMM routes (stride 1, the four stride-2 class launches, the class-concatenated form): dx = r(r(acc) + residual) - the fp32 sum
 *   is rounded to 16 bits, the residual added in fp32, the result rounded again;
 *   single-launch stride 2 (3x3, cin 32 / 64, cout 64, even maps, wo % 32 == 0; debug key 2 = 1 turns it off): dx = r(acc + residual) -
 *   one rounding after the sum and the residual;
 *   1x1 stride 2: the three parity classes the convolution never reads get the residual (or 0) copied. */
int mi355det_conv_dgrad(const mi355det_conv_shape* s, const void* dy, const void* wt, void* dx,
                        const void* residual, int32_t residual_ld, void* stream);

/* The same data gradient with a caller-owned workspace (replaces the same autograd step, torch/nn/grad.py conv2d_input as reached from
 * loss.backward() in detection/engine.py:49-57).  When the shape has few output pixels and a very deep reduction (stride 1, <= 96 tiles
 * of 128 x 128, k*k*cout >= 8192: the 1204-class RetinaNet head on the small pyramid levels, retinanet.py:75-105) the reduction is split
 * over channel ranges into fp32 partial tiles in `workspace` and added in a fixed order (deterministic; the bf16 rounding happens once,
 * after the sum and the residual: dx = r(acc + residual)).  mi355det_conv_dgrad_workspace returns the bytes that form needs, 0 when it does not apply; with a
 * NULL / zero workspace or a shape it does not apply to, conv_dgrad_ws IS conv_dgrad. */
/* Data gradient with the FrozenBatchNorm2d / ReLU backward of the layer that produced the convolution's input folded into the epilogue
 * (replaces, for a bottleneck's conv1 -> conv2 -> conv3 chain and the head towers, the autograd steps of F.relu and of the frozen affine,
 * utilities/resnet.py:107-125, tvision/backbone_utils.py:33-50, between two conv2d_input calls):
 *   dx = bf16(conv2d_input(dy)) * scale[c] * (act > 0)   (relu != 0)   |   bf16(conv2d_input(dy)) * scale[c]   (relu == 0)
 * act = the stored activation of that layer [n,h,w,cin] (pitch act_ld), scale [cin] or NULL.  Bit-identical to mi355det_conv_dgrad followed
 * by mi355det_relu_affine_bwd.  Stride-1 convolutions only. */
int mi355det_conv_dgrad_mask(const mi355det_conv_shape* s, const void* dy, const void* wt, void* dx, const void* act, int32_t act_ld,
                             const float* scale, int32_t relu, void* stream);
size_t mi355det_conv_dgrad_workspace(const mi355det_conv_shape* s);
int mi355det_conv_dgrad_ws(const mi355det_conv_shape* s, const void* dy, const void* wt, void* dx, const void* residual, int32_t residual_ld,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Data gradient that also starts the BatchNorm backward of the layer it feeds: dx is the gradient of an activation
 * a = lrelu(bn(z)); while the dx tile is still on chip the epilogue accumulates that layer's per-channel
 *   sum dy  and  sum dy*xhat,   dy = dx * lrelu'(z*scale+shift),  xhat = (z-mean)*invstd
 * into `partials` [rows+64][2][cin_pad] (plain stores, deterministic; rows = mi355det_conv_dgrad_bn_rows(s), the 64
 * spare rows are scratch), saving the separate bn_act_bwd_reduce pass its re-read of dx.  mi355det_bn_bwd_sum_partials
 * folds them into sums[2*cin] (same layout as bn_act_bwd_reduce).  scale_shift = [4*cin] of the producing layer. */
int mi355det_conv_dgrad_bn_rows(const mi355det_conv_shape* s);
int mi355det_conv_dgrad_bn(const mi355det_conv_shape* s, const void* dy, const void* wt, void* dx, const void* residual,
                           int32_t residual_ld, const void* z, int32_t z_ld, const float* scale_shift, float slope,
                           float* partials, void* stream);
int mi355det_bn_bwd_sum_partials(const float* partials, int32_t rows, int32_t c, int32_t c_pad, float* sums,
                                 void* stream);

/* Weight gradient: dw[cout][k*k*cin] fp32 += x^T dy.  Split over the pixel axis; partial 128x128 tiles go to
 * `workspace` with plain stores and are summed into dw in a fixed order: dw is bit-reproducible from run to run.
 * dbias != NULL: dbias[cout] += sum_pixels dy - this column sum ends in one fp32 atomicAdd per workgroup and channel,
 * so dbias (the three YOLO head biases, the RetinaNet / RPN head biases) is reproducible only to fp32 rounding order. */
size_t mi355det_conv_wgrad_workspace(const mi355det_conv_shape* s);
/* plan-build helper (synchronises; not part of the step): times the candidate split counts for this shape on the
 * caller's buffers and remembers the fastest.  Returns the chosen split count; dw is clobbered. */
int mi355det_conv_wgrad_autotune(const mi355det_conv_shape* s, const void* x, const void* dy, float* dw,
                                 void* workspace, size_t workspace_bytes, void* stream);
int mi355det_conv_wgrad(const mi355det_conv_shape* s, const void* x, const void* dy, float* dw,
                        float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* fp32 master weights, torch OIHW [cout][cin][k][k] or engine OHWI [cout][k][k][cin] (w_is_ohwi) -> bf16 fwd pack [cout_pad][k][k][cin] and
 * dgrad pack (stride 1: [cin_pad][k][k][cout] taps flipped; stride 2: 4 parity classes). */
size_t mi355det_dgrad_pack_elems(const mi355det_conv_shape* s);
int mi355det_pack_weights(const mi355det_conv_shape* s, const float* w, int w_is_ohwi, void* w_fwd,
                          int32_t cout_pad, void* w_dgrad, void* stream);
/* Batched form: all layers of a model re-packed by ONE launch per step.  The host table (entries + block table) is
 * built once from `items`, copied to the device by the caller, and replayed with mi355det_pack_weights_batched. */
typedef struct {
  const float* w;      /* device fp32 master */
  void* w_fwd;         /* device bf16 forward pack or NULL */
  void* w_dgrad;       /* device bf16 dgrad pack or NULL */
  mi355det_conv_shape shape;
  int32_t cout_pad, w_is_ohwi;
} mi355det_pack_item;
size_t mi355det_pack_table_bytes(const mi355det_pack_item* items, int32_t n, int32_t* n_entries, int32_t* n_blocks);
int mi355det_pack_table_build(const mi355det_pack_item* items, int32_t n, void* host_table, size_t host_bytes);
int mi355det_pack_weights_batched(const void* dev_table, int32_t n_entries, int32_t n_blocks, void* stream);
/* dw fp32 [cout][k][k][cin] -> torch layout [cout][cin][k][k] (param.grad) */
int mi355det_unpack_wgrad(const mi355det_conv_shape* s, const float* dw, float* grad, void* stream);

/* Grouped 3x3 convolution: conv2 of the ResNeXt Bottleneck (utilities/resnet.py: conv3x3(width, width, stride, groups), resnext50_32x4d /
 * resnext101_32x8d).  bf16 storage only.  s->cin == s->cout are the TOTAL channel counts, `groups` divides them.  Supported: ksize 3, pad 1,
 * stride 1 or 2, channels per group in {4, 8, 16, 32, 64}, cin a multiple of 32, any n / h / w and any pitches in_ld >= cin, out_ld >= cout
 * (16-byte accesses when base and pitch allow, 2-byte otherwise); pitch padding is never read or written.  Everything else returns
 * MI355DET_EINVAL before any launch.  Not a tuner candidate: one kernel per direction, no tune-record entries.
 *   gconv_pack_elems     bf16 elements of ONE operand image (forward and data-gradient image have the same size); 0 = unsupported shape
 *   gconv_pack_weights   fp32 masters [cout][3][3][cin/groups] (w_is_ohwi) or torch [cout][cin/groups][3][3] -> the block-diagonal forward
 *                        image (w_fwd) and / or the flipped, transposed data-gradient image (w_dgrad); either may be NULL.  Enqueued on
 *                        `stream`, no synchronisation (trainable layers repack every step)
 *   gconv_fwd_ex         y = relu?(conv(x, w) * scale + shift); e may be NULL; e->relu 0 or 1; a residual or out_f32 != 0 is MI355DET_EINVAL
 *   gconv_dgrad          dx [n,h,w,cin] (pitch in_ld) from dy [n,ho,wo,cout] (pitch out_ld): every element of dx is written, nothing is
 *                        accumulated
 *   gconv_wgrad          dw fp32 [cout][3][3][cin/groups] (the parameter-gradient layout) is WRITTEN, not accumulated: per-split partials go
 *                        to the workspace with plain stores and are added in split order - no atomics, bit-identical from call to call.
 *                        A workspace below mi355det_gconv_wgrad_workspace bytes returns MI355DET_EWORKSPACE. */
size_t mi355det_gconv_pack_elems(const mi355det_conv_shape* s, int32_t groups);
int mi355det_gconv_pack_weights(const mi355det_conv_shape* s, int32_t groups, const float* w, int w_is_ohwi, void* w_fwd, void* w_dgrad,
                                void* stream);
int mi355det_gconv_fwd_ex(const mi355det_conv_shape* s, int32_t groups, const void* x, const void* w_fwd, const mi355det_conv_epilogue* e,
                          void* y, int out_f32, void* stream);
int mi355det_gconv_dgrad(const mi355det_conv_shape* s, int32_t groups, const void* dy, const void* w_dgrad, void* dx, void* stream);
size_t mi355det_gconv_wgrad_workspace(const mi355det_conv_shape* s, int32_t groups);
int mi355det_gconv_wgrad(const mi355det_conv_shape* s, int32_t groups, const void* x, const void* dy, float* dw, void* workspace,
                         size_t workspace_bytes, void* stream);

/* BatchNorm2d (training) + LeakyReLU(0.1) around the conv (darknet.py:15-16,19-20):
 *   bn_finalize: stats -> scale/shift (+ running stats update, momentum 0.1, unbiased var).
 *   bn_act_fwd: a = lrelu(z*scale+shift) [+ residual]   (bf16 in/out, vectorised)
 *   bn_act_bwd_reduce: per-channel sums of dy and dy*xhat where dy = (g1[+g2]) * lrelu'(.)
 *   bn_act_bwd_apply: dz = scale*(dy - mean(dy) - xhat*mean(dy*xhat))  (bf16)
 * Limits and reproducibility:
 *   - c must be a multiple of 8 everywhere (MI355DET_EINVAL otherwise);
 *   - bn_act_bwd_reduce (legacy form) finishes every workgroup with one fp32 atomicAdd per channel into `sums`, so the two sums - and
 *     through them dz, dgamma, dbeta and everything upstream - differ from run to run in the last bits (measured ~6e-4 of max on the
 *     final gradient of a 75-layer step).  mi355det_bn_act_bwd_reduce_det below is the fixed-order form the engines use. */
int mi355det_bn_finalize(const float* stats, int32_t rows, int32_t c, int32_t c_pad, int64_t count,
                         const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var,
                         float* scale_shift /* [4*c]: scale, shift, mean, invstd */, void* stream);
/* SyncBN forward (apex convert_syncbn_model, yolo/procedures/initialize.py:31-32): the per-rank partial rows are folded in double
 * (exactly bn_finalize's own accumulation) into sums64 [2][c_pad] = (sum x | sum x*x), which the caller all-reduces as fp64 across the
 * ranks; bn_finalize_f64 then produces the same scale / shift / running statistics bn_finalize would from the global batch
 * (count = global element count per channel).  stats needs the 64 spare rows like bn_finalize. */
int mi355det_bn_fold_partials_f64(const float* stats, int32_t rows, int32_t c, int32_t c_pad, double* sums64, void* stream);
int mi355det_bn_finalize_f64(const double* sums64, int32_t c, int32_t c_pad, int64_t count, const float* gamma, const float* beta,
                             float eps, float momentum, float* running_mean, float* running_var, float* scale_shift,
                             void* stream);
/* eval mode (model.eval(), test_one_epoch.py:10): scale/shift from the running statistics */
int mi355det_bn_eval_scale_shift(int32_t c, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float eps, float* scale_shift, void* stream);
/* out = a + b on bf16 NHWC channel slices (gradient join of the concat/upsample branches) */
int mi355det_add_bf16(const void* a, int32_t a_ld, const void* b, int32_t b_ld, int32_t c, int64_t pixels,
                      void* out, int32_t out_ld, void* stream);
int mi355det_bn_act_fwd(const void* z, int32_t z_ld, const float* scale_shift, int32_t c, int64_t pixels,
                        float slope, const void* residual, int32_t res_ld, void* out, int32_t out_ld,
                        void* stream);
int mi355det_bn_act_bwd_reduce(const void* g1, int32_t g1_ld, const void* g2, int32_t g2_ld, const void* z,
                               int32_t z_ld, const float* scale_shift, int32_t c, int64_t pixels,
                               float slope, float* sums /* [2*c] zeroed by caller */, void* stream);
/* Fixed-order form of the same sums (what the engines use since round 4; reference: torch's batch_norm_backward is deterministic too,
 * yolo/nets/backbone/darknet.py:15-16): every workgroup stores its partial sums as one row of `workspace`, a second small launch adds the
 * rows in row order and WRITES sums[2*c] (no zeroing needed).  workspace: mi355det_bn_act_bwd_reduce_workspace(c, pixels) bytes, 16-byte
 * aligned, no initialisation; launches sharing a workspace must be ordered on one stream.  Bit-reproducible from run to run. */
size_t mi355det_bn_act_bwd_reduce_workspace(int32_t c, int64_t pixels);
int mi355det_bn_act_bwd_reduce_det(const void* g1, int32_t g1_ld, const void* g2, int32_t g2_ld, const void* z,
                                   int32_t z_ld, const float* scale_shift, int32_t c, int64_t pixels,
                                   float slope, float* sums, void* workspace, size_t workspace_bytes, void* stream);
int mi355det_bn_act_bwd_apply(const void* g1, int32_t g1_ld, const void* g2, int32_t g2_ld, const void* z,
                              int32_t z_ld, const float* scale_shift, const float* sums, const float* gamma,
                              int32_t c, int64_t pixels, float slope, void* dz, int32_t dz_ld,
                              float* dgamma, float* dbeta, void* stream);

/* nn.Upsample(scale_factor=2, nearest) into a channel slice (yolohead.py:32,80-81) and its adjoint */
int mi355det_upsample2x_fwd(const void* x, int32_t x_ld, int32_t n, int32_t h, int32_t w, int32_t c, void* out,
                            int32_t out_ld, void* stream);
int mi355det_upsample2x_bwd(const void* g, int32_t g_ld, int32_t n, int32_t h, int32_t w, int32_t c, void* out,
                            int32_t out_ld, void* stream);

/* ResNet stem as one direct convolution (utilities/resnet.py:173-176,232-234: conv1 7x7 / 2 / pad 3, 3 -> 64 + FrozenBatchNorm2d + ReLU;
 * the normalisation of tvision/transform.py:120-124 when mean / inv_std are given): replaces mi355det_im2col_nchw + the 160-deep GEMM of
 * mi355det_conv_fwd_ex for the frozen stem (no im2col matrix: 819 MB written and re-read at batch 16 / 800 px).  img [n,3,h,w] fp32,
 * w = the forward pack [64][160] bf16 (k = (kh*7+kw)*3 + c), scale / shift [64] or NULL, out [n, h/2, w/2, 64] bf16 (pitch out_ld).
 * h and w multiples of 32 (what GeneralizedRCNNTransform.batch_images pads to).  relu: bit 0 = ReLU; bits 1-3 are timing ablations of
 * tools/bench_rstem.py (skip the fragment compute / the halo fetch / the halo LDS store: wrong results) and must be 0 otherwise. */
int mi355det_resnet_stem_fwd(const float* img, const float* mean, const float* inv_std, const void* w, const float* scale,
                             const float* shift, int32_t relu, void* out, int32_t out_ld, int32_t n, int32_t h, int32_t wd,
                             void* stream);

/* ---- ResNet-FPN / RetinaNet elementwise companions (csrc/resnet_kernels.hip) -------------------------------------------
 * im2col_nchw: NCHW fp32 image, optional per-channel (x-mean)*inv_std (GeneralizedRCNNTransform.normalize,
 *   tvision/transform.py:120-124) -> rows [n*ho*wo][kpad] bf16, k=(kh*ks+kw)*c+ch: the 7x7/2 stem (resnet.py:173) runs
 *   as a 1x1 convolution with cin=kpad on the MFMA path.
 * maxpool3x3s2: nn.MaxPool2d(3,2,1) (resnet.py:176); _bwd: its adjoint (gradient to the first maximum of every window, gather form,
 *   deterministic) - needed when the 7x7 stem is trained (trainable_backbone_layers = 5, backbone_utils.py:100-104).
 * relu_affine_bwd: gm = (g1 [+g2]) * [a>0] (if relu), dz = gm * scale[c] (scale NULL = 1); gm / dz nullable.
 * upsample_nearest_add: out = lateral + interpolate(x, size=(out_h,out_w), nearest) (FPN top-down); _bwd its adjoint
 *   (out = accumulate + sum of g over the pixels that read it).
 * cast_rows_bf16: dst[b][r][0..cols) = src[b*image_stride + r*row_stride + c] * mul, zero fill up to dst_ld. */
int mi355det_im2col_nchw(const float* img, const float* mean, const float* inv_std, void* out, int32_t n, int32_t c,
                         int32_t h, int32_t w, int32_t ksize, int32_t stride, int32_t pad, int32_t kpad, void* stream);
int mi355det_maxpool3x3s2(const void* x, int32_t x_ld, int32_t n, int32_t h, int32_t w, int32_t c, void* out,
                          int32_t out_ld, void* stream);
int mi355det_maxpool3x3s2_bwd(const void* x, int32_t x_ld, const void* g, int32_t g_ld, int32_t n, int32_t h, int32_t w,
                              int32_t c, void* dx, int32_t dx_ld, void* stream);
int mi355det_relu_affine_bwd(const void* g1, int32_t g1_ld, const void* g2, int32_t g2_ld, const void* a, int32_t a_ld,
                             const float* scale, int32_t c, int64_t pixels, int relu, void* dz, int32_t dz_ld,
                             void* gm, int32_t gm_ld, void* stream);
int mi355det_upsample_nearest_add(const void* x, int32_t x_ld, int32_t n, int32_t h, int32_t w, int32_t c,
                                  const void* lateral, int32_t lateral_ld, int32_t out_h, int32_t out_w, void* out,
                                  int32_t out_ld, void* stream);
int mi355det_upsample_nearest_bwd(const void* g, int32_t g_ld, int32_t n, int32_t h, int32_t w, int32_t c, int32_t g_h,
                                  int32_t g_w, const void* accumulate, int32_t accumulate_ld, void* out,
                                  int32_t out_ld, void* stream);
int mi355det_cast_rows_bf16(const float* src, int64_t src_image_stride, int64_t src_row_stride, int32_t n, int64_t rows,
                            int32_t cols, float mul, void* dst, int32_t dst_ld, void* stream);

/* ---- fused optimizer step on the flat fp32 buffers --------------------------------------------------
 * Replaces torch.optim.SGD / Adam .step() (+ zero_grad) of yolo/procedures/initialize.py:38,41 and
 * yolo/procedures/train_one_epoch.py:96: one pass over {param, grad, state}.  grad_scale = 1/loss_scale (apex amp,
 * train_one_epoch.py:89) folded in.  first_step: momentum buffer is initialised with the gradient (torch semantics). */
int mi355det_sgd_step(float* w, float* g, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                      float weight_decay, float grad_scale, int nesterov, int first_step, int zero_grad, void* stream);
int mi355det_adam_step(float* w, float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, float grad_scale, int32_t step, int zero_grad,
                       void* stream);
/* The amp half of that row (apex `amp.scale_loss` + dynamic loss scaling around `optimizer.step()`, yolo/procedures/initialize.py:44-45,
 * train_one_epoch.py:88-96): grad_nonfinite sets *flag (device int32, zeroed by the caller) to 1 when any gradient is inf / nan (one read
 * pass); the *_guarded steps read *skip_flag on the device and leave parameters and optimizer state untouched when it is non-zero (the
 * gradients are still cleared when zero_grad is set), so an overflowing step is skipped without a host round trip.  skip_flag NULL = the
 * plain step. */
int mi355det_grad_nonfinite(const float* g, int64_t n, int32_t* flag, void* stream);
int mi355det_sgd_step_guarded(float* w, float* g, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                              float weight_decay, float grad_scale, int nesterov, int first_step, int zero_grad,
                              const int32_t* skip_flag, void* stream);
int mi355det_adam_step_guarded(float* w, float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, float grad_scale, int32_t step, int zero_grad,
                               const int32_t* skip_flag, void* stream);


/* ---- Fast R-CNN box-head loss (csrc/frcnn_kernels.hip) ------------------------------------------------------------------
 * Replaces `fastrcnn_loss` (torchvision_models/tvision/roi_heads.py:24-96) as RoIHeads.forward calls it (:826-827):
 *   fastrcnn_loss(tfidf * class_logits, box_regression, labels, regression_targets, weights=classification_weights, loss_type)
 * class_logits [n,k] fp32, box_regression [n,4k], labels [n] int64 (0 = background), regression_targets [n,4];
 * class_scale [k] or NULL = the tf-idf row multiplied into the logits; class_weights [k] or NULL ('ce' only);
 * loss_type 0 'ce', 1 'bce', 2 'focal_loss', 3 'gombit' (incl. its "/4 above 5" branch), 4 'gombit_fl'.
 * losses [2] = (loss_classifier, loss_box_reg); grad_logits [n,k] / grad_box [n,4k] (nullable) = d(loss_classifier)/d(class_logits)
 * (UNSCALED logits) and d(loss_box_reg)/d(box_regression).  Deterministic (no atomics).  Returns EINVAL for n < 1, k < 2, a loss_type
 * outside 0..4 or class weights with a loss other than 'ce'. */
size_t mi355det_fastrcnn_loss_workspace(int32_t n);
int mi355det_fastrcnn_loss(const float* class_logits, const float* box_regression, const int64_t* labels,
                           const float* regression_targets, const float* class_scale, const float* class_weights, int32_t n,
                           int32_t k, int32_t loss_type, float* losses, float* grad_logits, float* grad_box, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- Long-tail baselines (csrc/longtail_kernels.hip) ---------------------------------------------------------
 * The three standard LVIS baselines the tf-idf method is judged against, restated from the papers (nothing is run against mmdetection
 * or detectron2): Seesaw loss, Equalization loss v1 and repeat-factor sampling.
 *
 * label_histogram: counts[labels[i]] += 1 for i < n with unsigned 64-bit integer atomics (exact, the same from run to run); counts [k]
 *   int64 is NOT cleared first (it is Seesaw's cumulative state).  A label outside [0, k) is skipped.
 *
 * fastrcnn_loss_longtail: the operands of mi355det_fastrcnn_loss (no class weights) with its own loss_type, 0 'seesaw' or 1 'eql'.
 *   x = class_scale * logits, column 0 is the background, gradients are w.r.t. the UNSCALED logits, the box loss is the smooth-L1 of
 *   mi355det_fastrcnn_loss (the same device code).
 *   seesaw (p, q, eps; the paper's 0.8, 2, 1e-2): counts [k] int64 = rows seen per label so far, background included.  With update_counts
 *     != 0 the histogram of `labels` is added to counts BEFORE the loss reads it.  N_c = max(counts[c], 1), s = softmax(x) (no gradient);
 *     for a row labelled y and every column j:  M_j = (N_j / N_y)^p if N_j < N_y else 1;  r_j = s_j / max(s_y, eps), C_j = r_j^q if r_j > 1
 *     else 1;  x'_j = x_j + log(M_j C_j), both factors 1 at j = y;  loss = mean over rows of logsumexp(x') - x'_y;
 *     d loss / d logits_j = class_scale_j (softmax(x')_j - [j = y]) / n (M and C are constants).
 *   eql: tail [k] uint8, 1 = a tail category (tail[0] must be 0: the caller checks).  t_j = [j = y and j != 0] (the 'bce' targets),
 *     w_j = 1 - [y > 0] tail_j (1 - t_j);  loss = sum_rows sum_j w_j BCEWithLogits(x_j, t_j) / n;
 *     d loss / d logits_j = class_scale_j w_j (sigmoid(x_j) - t_j) / n.
 *   A label outside [0, k) is never used as an index: that row's class loss is NaN (and so is losses[0]), its gradients are 0 and it adds
 *   nothing to counts.  Deterministic: no float atomics.  Returns EINVAL for n < 1, k < 2, a loss_type outside 0..1, counts == NULL with
 *   seesaw or tail == NULL with eql, p or q negative or not finite, eps outside (0, 1]; EWORKSPACE for a workspace below
 *   fastrcnn_loss_longtail_workspace(n, k).
 *
 * repeat_factors: one (image, category) index pair per annotation (mi355det_category_frequencies' operands) and that call's img_freq
 *   [n_categories] -> r_image [n_images] float64, which the CALLER pre-fills with 1.0:  f_c = img_freq[c] / n_images,
 *   r_c = max(1, sqrt(t / f_c)) in float64, r_image[i] = max over the annotations of image i of r_c, written with a 64-bit integer
 *   atomic maximum on the bit pattern (non-negative doubles order as unsigned integers: the result does not depend on the order).
 *   errors [1] int32 counts the annotations with an index outside its range; they are skipped. */
int mi355det_label_histogram(const int64_t* labels, int32_t n, int32_t k, int64_t* counts, void* stream);
size_t mi355det_fastrcnn_loss_longtail_workspace(int32_t n, int32_t k);
int mi355det_fastrcnn_loss_longtail(const float* class_logits, const float* box_regression, const int64_t* labels,
                                    const float* regression_targets, const float* class_scale, int32_t n, int32_t k, int32_t loss_type,
                                    int64_t* counts, const uint8_t* tail, float p, float q, float eps, int32_t update_counts, float* losses,
                                    float* grad_logits, float* grad_box, void* workspace, size_t workspace_bytes, void* stream);
int mi355det_repeat_factors(const int32_t* image_index, const int32_t* category_index, int64_t n_annotations, const int32_t* img_freq,
                            int32_t n_images, int32_t n_categories, double t, double* r_image, int32_t* errors, void* stream);

/* ---- input-side transform (csrc/transform_kernels.hip) -------------------------------------------------
 * resize_bilinear: `planes` fp32 planes [planes][h][w] -> out [planes][pad_h][pad_w]: F.interpolate(mode='bilinear', align_corners=False)
 *   to (out_h, out_w) with the sampling scale taken from the two sizes (recompute_scale_factor=True / size=...), zeros in the pad.
 *   mean/std [c] (nullable together): (x - mean[p % c]) / std[p % c] applied to the taps = GeneralizedRCNNTransform.normalize followed by
 *   resize and batch_images (torchvision_models/tvision/transform.py:120-135,215-226) for one image (planes = c = 3) written into its slot
 *   of the padded batch; with mean = NULL and planes = N*C it is the YOLO multi-scale resize (yolo/procedures/train_one_epoch.py:64-69).
 * resize_boxes: transform.py:279-293, boxes [n,4] xyxy scaled by float32 ratios new/orig. */
int mi355det_resize_bilinear(const float* in, int32_t planes, int32_t c, int32_t h, int32_t w, const float* mean, const float* stdv,
                             float* out, int32_t out_h, int32_t out_w, int32_t pad_h, int32_t pad_w, void* stream);
int mi355det_resize_boxes(const float* boxes, float* out, int64_t n, int32_t orig_h, int32_t orig_w, int32_t new_h, int32_t new_w,
                          void* stream);

/* ---- batched uint8 ingest (csrc/transform_kernels.hip): decoded images to the padded batch in one launch ---------------------
 * The route of GeneralizedRCNNTransform for images as a decoder hands them over: uint8 [h, w, 3] (HWC), any sizes, packed back to back
 * into one buffer.  One table entry per image; the same table is read by the host checks (`table`, host memory) and by the kernels
 * (`table_dev`, the caller's device copy of it).
 *   ingest_u8          out fp32 [n, 3, pad_h, pad_w], every element written once (zeros outside [out_h, out_w]): the horizontal flip of
 *                      detection/transforms.py:30-34 (a flipped image reads source column w - 1 - x), ToTensor's byte / 255 (a correctly
 *                      rounded division), normalize, bilinear resize and batch_images with the arithmetic of mi355det_resize_bilinear
 *                      (one blend function serves both), so the result equals, bit for bit, mi355det_resize_bilinear of the flipped float
 *                      image.  A block owns tiles of MI355DET_INGEST_TILE_H x MI355DET_INGEST_TILE_W output pixels of one image and finds
 *                      the image by a search of first_tile; image i owns the tiles [first_tile[i], first_tile[i] + mi355det_ingest_tiles).
 *                      mean / stdv: device fp32 [3].  EINVAL for n <= 0, a null pointer, h, w, out_h, out_w <= 0, pad < out, an image
 *                      that does not lie inside [0, packed_bytes) or a first_tile column that is not i * mi355det_ingest_tiles(pad_h,
 *                      pad_w) (0 when the count does not fit).
 *   flip_resize_boxes  all images' boxes in one launch: boxes [g, 4] xyxy concatenated, box_offsets int64 [n + 1] on the device (image i
 *                      owns rows [box_offsets[i], box_offsets[i + 1])).  Where the image is flipped, x0' = w - x2 and x2' = w - x0 in
 *                      float32 (transforms.py:37); then the ratio multiply of mi355det_resize_boxes with the same float32 ratios
 *                      out / in.  g == 0 is a no-op. */
#define MI355DET_INGEST_TILE_H 16
#define MI355DET_INGEST_TILE_W 64
typedef struct {
  int64_t offset;     /* byte offset of the image's [h, w, 3] bytes in the packed buffer */
  int32_t h, w;       /* source size */
  int32_t out_h, out_w; /* resized size, <= the pad */
  int32_t flip;       /* != 0: mirrored left to right */
  int32_t first_tile; /* index of the image's first tile in the launch */
} mi355det_ingest_image;
int32_t mi355det_ingest_tiles(int32_t pad_h, int32_t pad_w);
int mi355det_ingest_u8(const uint8_t* packed, int64_t packed_bytes, const mi355det_ingest_image* table,
                       const mi355det_ingest_image* table_dev, int32_t n, const float* mean, const float* stdv, float* out, int32_t pad_h,
                       int32_t pad_w, void* stream);
int mi355det_flip_resize_boxes(const float* boxes, float* out, int64_t g, const int64_t* box_offsets,
                               const mi355det_ingest_image* table_dev, int32_t n, void* stream);

/* ---- SSD augmentations of the uint8 ingest (csrc/augment_kernels.hip): detection/transforms.py:54-239 on the packed bytes ------
 * The reference's `ssd` and `ssdlite` policies (detection/presets.py:12-25) run on PIL images, so every stage is Pillow's 8-bit
 * arithmetic.  The host decides (tvision/transforms.py) and hands over tables; the kernels apply.
 *
 * photometric_u8: RandomPhotometricDistort, in place on the packed bytes.  One entry per image THAT HAS OPS (m <= n), at most
 * MI355DET_PHOTO_MAX_OPS ops in order and then a channel permutation.  The rules, per pixel (R, G, B):
 *   blend(d, v, f)  t = d + f * (v - d) with f and the arithmetic in float32, clipped to [0, 255], truncated (Image.blend)
 *   L               (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 *   BRIGHTNESS      blend(0, v, f) on each byte
 *   CONTRAST        blend(D, v, f) with D = int(sum / pixels + 0.5) in float64, sum the integer sum of L over the whole image as it is
 *                   after the ops in front; at most one per image.  A launch of its own forms the sums (`sums`, m device words that
 *                   the entry clears), the applying launch forms D: no host read between them
 *   SATURATION      blend(L, v, f) on each byte, L of the same pixel
 *   HUE             RGB -> HSV, H = (H + shift) mod 256, HSV -> RGB.  factor carries the shift, np.uint8(hue_factor * 255), as a whole
 *                   number in [0, 255].  RGB -> HSV: V = max; S = int(255 * s), s = cr / max in float32, cr = max - min; the three
 *                   quotients (max - c) / cr in float32, h = bc - gc, 2 + rc - bc or 4 + gc - rc (in float64, rounded to float32),
 *                   h = fmod(h / 6 + 1, 1) in float64, rounded to float32, H = int(255 * h); grey has H = S = 0.  HSV -> RGB: S == 0
 *                   gives grey; else h = H * 6 / 255, i = floor(h), f = h - i, s = S / 255, p, q, t = round(V (1 - s)),
 *                   round(V (1 - s f)), round(V (1 - s (1 - f))) in float64, the six cases of colorsys by i mod 6
 *   perm            output channel c is channel perm[c] of the result (identity: 0, 1, 2)
 * Image i owns the blocks [first_block, first_block + mi355det_photo_blocks(pixels)), MI355DET_PHOTO_BLOCK_PIXELS pixels each.
 * EINVAL, before any launch, for m <= 0, a null pointer, an image outside the packed bytes, n_ops outside [0, MAX_OPS], an op code out of
 * range, a factor that is negative or not finite (a hue shift that is no whole number in [0, 255]), two contrast ops in one image, a
 * perm that is no permutation, or a first_block column that is not the running sum of the block counts.
 *
 * ingest_aug_u8: mi355det_ingest_u8 with one other rule for fetching a tap (one tile loop serves both: csrc/ingest_body.h).  The
 * resize sees a window [crop_h, crop_w] at (crop_top, crop_left) of a canvas [canvas_h, canvas_w] on which the source image is pasted at
 * (paste_top, paste_left) and whose other pixels are `fill` (RandomZoomOut; without it the canvas is the image, pasted at 0, 0;
 * RandomIoUCrop's window; without it the whole canvas).  A tap (y, x) of the window reads canvas pixel (crop_top + y, crop_left + x'),
 * x' = crop_w - 1 - x where the image is flipped: three source bytes or the three fill bytes.  The canvas is never stored.  Sizes, scale
 * and out_h / out_w are those of the window.  EINVAL, before any launch, for what ingest_u8 refuses and for a pasted image outside its
 * canvas, a crop outside its canvas and a window with a zero side.  mi355det_flip_resize_boxes then takes a table of
 * mi355det_ingest_image whose h, w are the windows'. */
#define MI355DET_PHOTO_MAX_OPS 5
#define MI355DET_PHOTO_BLOCK_PIXELS 4096
#define MI355DET_PHOTO_BRIGHTNESS 1
#define MI355DET_PHOTO_CONTRAST 2
#define MI355DET_PHOTO_SATURATION 3
#define MI355DET_PHOTO_HUE 4
typedef struct {
  int64_t offset;      /* byte offset of the image's [h, w, 3] bytes in the packed buffer */
  int64_t pixels;      /* h * w */
  int32_t first_block; /* index of the image's first block in the launch */
  int32_t n_ops;
  int32_t op[MI355DET_PHOTO_MAX_OPS];
  float factor[MI355DET_PHOTO_MAX_OPS];
  int32_t perm[3];
  int32_t reserved;
} mi355det_photo_image;
typedef struct {
  int64_t offset;                 /* byte offset of the source image's [h, w, 3] bytes in the packed buffer */
  int32_t h, w;                   /* source size */
  int32_t canvas_h, canvas_w;     /* the zoom-out canvas; h, w without one */
  int32_t paste_top, paste_left;  /* where the source image lies on the canvas */
  int32_t crop_top, crop_left;    /* the window of the canvas that the resize sees */
  int32_t crop_h, crop_w;
  int32_t out_h, out_w;           /* resized size of the window, <= the pad */
  int32_t flip;                   /* != 0: the window is mirrored left to right */
  int32_t first_tile;             /* index of the image's first tile in the launch */
  uint32_t fill_rgb;              /* the canvas outside the pasted image: R | G << 8 | B << 16 */
  int32_t reserved;
} mi355det_ingest_aug_image;
int32_t mi355det_photo_blocks(int64_t pixels);
int mi355det_photometric_u8(uint8_t* packed, int64_t packed_bytes, const mi355det_photo_image* table,
                            const mi355det_photo_image* table_dev, int32_t m, uint64_t* sums, void* stream);
int mi355det_ingest_aug_u8(const uint8_t* packed, int64_t packed_bytes, const mi355det_ingest_aug_image* table,
                           const mi355det_ingest_aug_image* table_dev, int32_t n, const float* mean, const float* stdv, float* out,
                           int32_t pad_h, int32_t pad_w, void* stream);

/* ---- YOLO ingest (csrc/cubic_kernels.hip): decoded uint8 images through OpenCV's bicubic resize to the square batch -----------
 * The YOLO twin of the uint8 ingest above: yolo/dsets/transformations.py:10-53 (ResizeToTensor = cv2.resize(img, (S, S), INTER_CUBIC),
 * / 255, normalise, boxes to relative xcycwh) for a whole batch, one launch for the images and one for the boxes.
 *
 * The rule is OpenCV's 8-bit INTER_CUBIC path, restated from resize.cpp (the C path; a SIMD build of OpenCV may round the last bit
 * differently).  Each output axis maps a source size `src` to a destination size `dst` on its own.  For an output index d:
 *   scale    scale = 1.0 / (dst / (double)src)
 *   position fx = (float)((d + 0.5) * scale - 0.5), the product in double
 *   split    s = floor(fx), then fx -= s in float32
 *   weights  float32, A = -0.75, every expression evaluated as written:
 *              c0 = ((A*(fx+1) - 5A)*(fx+1) + 8A)*(fx+1) - 4A
 *              c1 = ((A+2)*fx - (A+3))*fx*fx + 1
 *              c2 = ((A+2)*(1-fx) - (A+3))*(1-fx)*(1-fx) + 1
 *              c3 = 1 - c0 - c1 - c2, left to right
 *   fixed    w_k = (short)rint(c_k * 2048): a float32 product, rounded half to even, saturated to int16; not renormalised
 *   taps     source indices s-1 .. s+2, each clamped to [0, src-1]; no antialiasing, whatever the scale
 *   pixel    per channel acc = sum_ky wy[ky] * (sum_kx wx[kx] * S[y_ky][x_kx]) in int32 (|acc| < 2^31 for every weight the rule can
 *            give: the |w_k| of an axis sum to at most 2816 + 2, at fx = 0.5, and 2818 * 2818 * 255 < 2^31), integers, so any order
 *            gives the same bits
 *   byte     clamp((acc + (1 << 21)) >> 22, 0, 255), an arithmetic shift
 *   grey     a [h, w] image is its channel three times (cv2.cvtColor(GRAY2RGB), transformations.py:30-34)
 *   flip     a flipped image reads source column w - 1 - x (the project's own addition, as in the ingest above)
 *   value    float32((float32(byte / 255.0 in float64) - mean_c) / std_c): 768 values, which the caller builds on the host with the
 *            reference's own operations (transformations.py:36-41) and hands over as `lut`
 * The (s, w0..w3) of an axis depend on (src, dst) alone.  The caller builds them on the host in the order above and uploads them (`taps`);
 * the kernel does no float arithmetic at all, so nothing on the device has to round as the host does.
 *   yolo_ingest_u8  out fp32 [n, 3, size, size], every element written once.  packed: the images' bytes back to back ([h, w, 3], or
 *                   [h, w] where channels == 1); table / table_dev: one entry per image, host copy for the checks and device copy for
 *                   the kernel; taps_dev: n_taps entries on the device, image i reads [xtab, xtab + size) for its columns and
 *                   [ytab, ytab + size) for its rows; lut: device fp32 [3][256].  The kernel clamps every tap index itself, so no
 *                   content of `taps_dev` can make it read outside an image.  EINVAL, before any launch, for n <= 0, a null pointer,
 *                   size <= 0, h or w <= 0, channels other than 1 or 3, an image that does not lie inside [0, packed_bytes) or an
 *                   xtab / ytab with [tab, tab + size) outside [0, n_taps).
 *   yolo_targets    all images' boxes in one launch: boxes float64 [g, 4] (xmin, ymin, w, h) and area float64 [g] concatenated,
 *                   box_offsets int64 [n + 1] on the device as for flip_resize_boxes.  In float64 (transformations.py:44-49,
 *                   helper.convert2_rel_xcycwh): where the image is flipped xmin' = w - (xmin + bw) first; xc = xmin / w + (bw / w) / 2,
 *                   yc = ymin / h + (bh / h) / 2, bw / w, bh / h, cast to float32 into bbox [g, 4]; rel_area [g] = area / (h * w) stays
 *                   float64.  EINVAL for n <= 0, g < 0 or a null pointer; g == 0 is a no-op. */
#define MI355DET_YOLO_TILE_H 16
#define MI355DET_YOLO_TILE_W 64
typedef struct {
  int32_t s;     /* floor of the source position: the taps are s-1 .. s+2 */
  int16_t w[4];  /* the weights in units of 1/2048 */
} mi355det_cubic_tap;
typedef struct {
  int64_t offset;     /* byte offset of the image's bytes in the packed buffer */
  int32_t h, w;       /* source size */
  int32_t channels;   /* 3: [h, w, 3]; 1: [h, w], grey */
  int32_t flip;       /* != 0: mirrored left to right */
  int32_t xtab, ytab; /* index of the image's first column / row entry in the tap buffer */
} mi355det_yolo_image;
int mi355det_yolo_ingest_u8(const uint8_t* packed, int64_t packed_bytes, const mi355det_yolo_image* table,
                            const mi355det_yolo_image* table_dev, int32_t n, const mi355det_cubic_tap* taps_dev, int64_t n_taps,
                            const float* lut, float* out, int32_t size, void* stream);
int mi355det_yolo_targets(const double* boxes, const double* area, int64_t g, const int64_t* box_offsets,
                          const mi355det_yolo_image* table_dev, int32_t n, float* bbox, double* rel_area, void* stream);

/* ---- output side: detections -> the numbers of the COCO json dicts (csrc/transform_kernels.hip) ----------
 * yolo/procedures/test_one_epoch.py:41-66 (scale = 1): boxes rows (x1,y1,x2,y2,...) with pitch box_ld in network pixels ->
 *   bbox_xywh [k,4] = (x1/inp_dim*W, y1/inp_dim*H, w, h) in the original image, area [k] = w*h, category_id [k] from the label column
 *   (labels_f32 with pitch label_ld, cast like `.long()`, or labels_i64): label_mode 0 = label + 1, 1 = COCO 80 -> 91 map
 *   (yolo/utilities/helper.py:16-24), 2 = unchanged.
 * torchvision_models/detection/coco_eval.py:83-105,169-171 (scale = 0, label_mode 2): convert_to_xywh.  area / category_id nullable. */
int mi355det_coco_rows(const float* boxes, int32_t box_ld, const float* labels_f32, const int64_t* labels_i64, int32_t label_ld,
                       int64_t k, float inp_dim, float img_h, float img_w, int32_t scale, int32_t label_mode, float* bbox_xywh,
                       float* area, int64_t* category_id, void* stream);

/* ---- Mask R-CNN mask branch (csrc/mask_kernels.hip; tvision/mask_rcnn.py:21-300, tvision/roi_heads.py:99-183,403-537,844-887).  bf16
 * storage, fp32 arithmetic; the R-CNN path is bf16-only, so these have no fp16 twins.  The ConvTranspose2d(256, 256, 2, stride=2) of the
 * predictor is the 1x1 convolution 256 -> 1024 of mi355det_conv_fwd_ex / _dgrad_mask / _wgrad (output channel q*256 + co, q = 2*di + dj:
 * kernel == stride, so output pixel (2i+di, 2j+dj) reads input pixel (i, j) only); its output stays in that sub-pixel order
 * [R, 14, 14, 4*256] and mask_loss / mask_probs index the 28 x 28 mask through it.
 *   mask_roi_pool        MultiScaleRoIAlign(['0'..'3'], 14, 2) (roi_heads mask_roi_pool) writing bf16 NHWC [R, ph, pw, C] with pixel pitch
 *                        out_ld: out == bf16(mi355det_roi_align_nhwc) bit for bit.  Backward (grad_out != NULL, bf16 NHWC with pitch
 *                        grad_ld): scatters into grad_feats (dense fp32 NHWC, zeroed by the caller) with fp32 atomics, like the box branch.
 *   mask_targets         project_masks_on_boxes (roi_heads.py:131-144): roi_align(gt_masks[:, None].float(), rois, (m, m), 1.0), sampling -1,
 *                        aligned False, all images in one launch: rois [R, 5] = (image, box), gt_index [R] = matched gt WITHIN the image,
 *                        images->masks[b] = uint8 [G_b, h[b], w[b]] (NULL for an image no RoI refers to).  out fp32 [R, m, m].
 *   mask_loss            maskrcnn_loss (roi_heads.py:147-183) fused with mask_fcn_logits (1x1, 256 -> K) on the label channel only: feat = the
 *                        deconvolution output after its ReLU (bf16, sub-pixel order, pitch feat_ld >= 1024), w_logits [K, 256] / b_logits [K]
 *                        fp32, labels [rows] int64, targets [rows, 28, 28].  rows = the bucket (padded), valid = the real positives: rows
 *                        >= valid get zero gradient.  loss[0] = mean BCE-with-logits over valid*784 elements; dfeat = d loss / d (deconv
 *                        pre-activation) (its ReLU folded in, bf16, same layout); dw [K, 256] / db [K] / dbias_deconv [256] are fixed-order
 *                        reductions of per-RoI partials (no atomics, bit-reproducible); every class row is written.  valid == 0: loss 0
 *                        and zero gradients.  workspace: mi355det_mask_loss_workspace(rows) bytes.
 *   mask_probs           maskrcnn_inference (roi_heads.py:99-128): probs [rows, 28, 28] = sigmoid of the label channel.
 *   mask_resize_nearest _resize_image_and_masks, masks part (transform.py:54-60): uint8 [planes, h, w] -> [planes, out_h, out_w], torch's
 *                        nearest source index (same size: copy; doubling: dst >> 1; else min(floor(dst * (float)in / out), in - 1)).
 *   paste_masks          paste_masks_in_image (roi_heads.py:517-537): masks fp32 [D, m, m], boxes [D, 4] in the original image; expand_masks
 *                        (padding) + expand_boxes + int64 truncation + bilinear resize (align_corners False) + clipped paste -> out fp32
 *                        [D, im_h, im_w], every pixel written once. */
#define MI355DET_MASK_MAX_IMAGES 64
typedef struct {
  const uint8_t* masks[MI355DET_MASK_MAX_IMAGES];
  int32_t h[MI355DET_MASK_MAX_IMAGES];
  int32_t w[MI355DET_MASK_MAX_IMAGES];
  int32_t n_images;
} mi355det_mask_images;
int mi355det_mask_roi_pool(const void* const* feats, const int32_t* hs, const int32_t* ws, const int32_t* lds, const float* scales,
                           int32_t num_levels, const float* rois, int32_t num_rois, int32_t channels, int32_t pooled_h, int32_t pooled_w,
                           int32_t sampling_ratio, int32_t k_min, int32_t k_max, void* out, int32_t out_ld, const void* grad_out,
                           int32_t grad_ld, float* const* grad_feats, void* stream);
int mi355det_mask_targets(const mi355det_mask_images* images, const float* rois, const int64_t* gt_index, int32_t num_rois, int32_t m,
                          float* out, void* stream);
size_t mi355det_mask_loss_workspace(int32_t rows);
int mi355det_mask_loss(const void* feat, int32_t feat_ld, const float* w_logits, const float* b_logits, const int64_t* labels,
                       const float* targets, int32_t rows, int32_t valid, int32_t num_classes, float* loss, void* dfeat, float* dw,
                       float* db, float* dbias_deconv, void* workspace, size_t workspace_bytes, void* stream);
int mi355det_mask_probs(const void* feat, int32_t feat_ld, const float* w_logits, const float* b_logits, const int64_t* labels, int32_t rows,
                        int32_t num_classes, float* probs, void* stream);
int mi355det_mask_resize_nearest(const uint8_t* in, int32_t planes, int32_t h, int32_t w, uint8_t* out, int32_t out_h, int32_t out_w,
                                 void* stream);
/* mask_resize_nearest of masks.flip(-1) when flip != 0 (detection/transforms.py:38-39 ahead of the resize): source column w - 1 - x. */
int mi355det_mask_flip_resize_nearest(const uint8_t* in, int32_t planes, int32_t h, int32_t w, uint8_t* out, int32_t out_h, int32_t out_w,
                                      int32_t flip, void* stream);
int mi355det_paste_masks(const float* masks, const float* boxes, int32_t num_masks, int32_t m, int32_t padding, int32_t im_h, int32_t im_w,
                         float* out, void* stream);

/* ---- Mask results as COCO run-length encodings (csrc/rle_kernels.hip, csrc/rle_codec.cpp; torchvision_models/detection/coco_eval.py:107-140
 * prepare_for_coco_segmentation = `masks > 0.5` + pycocotools mask.encode + counts.decode).  Run lengths follow pycocotools rleEncode: the
 * pixels of one mask in column-major order i = x*im_h + y, counts = lengths of alternating runs beginning with a run of zeros (which may be
 * 0), so an all-zero mask is [im_h*im_w], an all-one mask [0, im_h*im_w], and a run goes on from the bottom of one column into the top of
 * the next.  A mask with T transitions has T + 1 counts.  Two sources of the bit at (d, y, x), chosen by `dense`:
 *   dense != NULL   dense[d][y][x] > threshold for fp32 [D, im_h, im_w] (the reference's contract: pasted masks); masks / boxes unused.
 *   dense == NULL   the value mi355det_paste_masks would write at (d, y, x) (same float32 bits: csrc/mask_paste.h) > threshold, from the
 *                   m x m probabilities masks [D, m, m] and boxes [D, 4]; the full-size mask is never stored, and only the columns and
 *                   rows of the clipped box are evaluated (outside it the bit is 0, hence threshold >= 0 is required).
 *   mask_rle_count  counts every column's transitions and scans them: run_offsets [D + 1] int64 on the device (run_offsets[d] = index of
 *                   mask d's first count, run_offsets[D] = the number of counts in all), and leaves the column tables in the workspace.
 *   mask_rle_emit   needs the workspace mask_rle_count left for the SAME source: writes counts [run_offsets[D]] int32, area [D] int64
 *                   (set pixels = the sum of the odd-indexed counts; pycocotools area) and bbox [D, 4] int32 = [xmin, ymin, xmax - xmin + 1,
 *                   ymax - ymin + 1] of the set pixels, zeros for an empty mask (pycocotools toBbox); area / bbox nullable.  total_runs is
 *                   the caller's host copy of run_offsets[D] (it sizes counts by it anyway); capacity < total_runs is an error, and no
 *                   count is ever written at an index >= capacity.
 * No atomics; the output is bit-identical from run to run.  im_h*im_w must be below 2^31.  workspace: mi355det_mask_rle_workspace bytes.
 *   rle_to_string / rle_from_string   pycocotools rleToString / rleFrString on the host (no GPU call): each count (from the fourth on, its
 *                   difference to the count two before) as 5-bit groups, low group first, bit 0x20 = more groups follow, char = group + 48.
 *                   to_string writes the characters and a terminating NUL and returns the number of characters; out == NULL only sizes.
 *                   from_string returns the number of counts; counts == NULL only sizes.  A negative status when cap is too small (nothing
 *                   is written past cap) or the string is malformed. */
size_t mi355det_mask_rle_workspace(int32_t num_masks, int32_t im_w);
int mi355det_mask_rle_count(const float* dense, const float* masks, const float* boxes, int32_t num_masks, int32_t m, int32_t padding,
                            int32_t im_h, int32_t im_w, float threshold, int64_t* run_offsets, void* workspace, size_t workspace_bytes,
                            void* stream);
int mi355det_mask_rle_emit(const float* dense, const float* masks, const float* boxes, int32_t num_masks, int32_t m, int32_t padding,
                           int32_t im_h, int32_t im_w, float threshold, const int64_t* run_offsets, int64_t total_runs, int32_t* counts,
                           int64_t capacity, int64_t* area, int32_t* bbox, void* workspace, size_t workspace_bytes, void* stream);
int64_t mi355det_rle_to_string(const int32_t* counts, int64_t n, char* out, int64_t cap);
int64_t mi355det_rle_from_string(const char* s, int32_t* counts, int64_t cap);

/* ---- Keypoint R-CNN keypoint branch (csrc/keypoint_kernels.hip): tvision/roi_heads.py:186-379,891-932, the keypoint parts of
 * tvision/transform.py:169-172,244-275 and detection/transforms.py:10-19.  The head (8 x Conv2d 3x3 + ReLU) and the transposed
 * convolution run on the convolution entries above; ConvTranspose2d(512, K, 4, 2, 1) as a 3x3 / padding 1 convolution to 4 * KP channels
 * with fp32 output.  SUB-PIXEL LAYOUT of its output and of the gradient that comes back: [rows, 14, 14, ld], channel (2a + b) * KP + k of
 * pixel (i, j) = keypoint k at pixel (2i + a, 2j + b) of the 28 x 28 map; KP >= K (padded channels: zero weights, zero gradients).
 *   flip_resize_keypoints  keypoints fp32 [g, K, 3] of a whole batch, image b owning rows [kp_offsets[b], kp_offsets[b + 1]) (int64
 *                          [n + 1] ON THE DEVICE), table (host) and table_dev (its device copy) as for mi355det_ingest_u8.  Flipped image:
 *                          _flip_coco_person_keypoints (the COCO left/right index permutation of 17 indices: EINVAL, before the launch,
 *                          where a table entry has flip set and K != 17;
 *                          x = w - x, the triple zeroed where v == 0); then resize_keypoints: x * (out_w / w), y * (out_h / h) with
 *                          float32 ratios, v untouched.
 *   keypoint_targets       keypoints_to_heatmap for all RoIs in one launch: rois [rows, 5] = (image, x1, y1, x2, y2), gt_index [rows]
 *                          int64 = matched ground truth inside the image, keypoints / kp_offsets as above ->
 *                          target int32 [rows, K] = y * size + x (0 where not valid), valid int32 [rows, K], count int32 [1] = number of
 *                          valid pairs, left on the device.  Float32 in the reference's order: floor((x - x1) * (size / (x2 - x1))), IEEE
 *                          division; x == x2 (y == y2) -> size - 1; valid = inside [0, size)^2 and v > 0.  Rows >= valid_rows (bucket
 *                          padding) and matches outside their image's keypoints are not valid.
 *   keypoint_heatmaps      logits fp32 in the sub-pixel layout -> out fp32 [rows, K, 56, 56]: F.interpolate(scale_factor=2, bilinear,
 *                          align_corners=False) (source (d + 0.5) / 2 - 0.5 clamped at 0: weights 0.25 / 0.75).
 *   keypoint_loss          keypointrcnn_loss on those 56 x 56 logits, formed on the fly: loss [1] = mean over the valid pairs of
 *                          logsumexp - logit[target]; dlogits bf16 in the sub-pixel layout (pitch logits_ld; all of it is written, zeros
 *                          in padded channels) = the gradient (softmax - onehot) / count gathered back through the x2, each low-resolution
 *                          cell summing its at most 16 contributors in a fixed order; dlogits_f32 (nullable) fp32 [rows, K, 28, 28] =
 *                          that gradient before its rounding to bf16; dbias [K] = the transposed convolution's bias
 *                          gradient.  count is read on the device.  No float atomics, bit-identical from run to run.  rows == 0 or
 *                          count == 0: loss 0 and zero gradients.  workspace: mi355det_keypoint_loss_workspace bytes; on return it holds, as
 *                          fp32 [rows, K, 2], every pair's loss term lse - logit[target] (0 where not valid) and the sum of its gradient.
 *   heatmaps_to_keypoints  maps fp32 [rows, K, 56, 56], rois [rows, roi_ld] (roi_ld 4: box; 5: (image, box)) -> xy fp32 [rows, K, 3],
 *                          scores fp32 [rows, K], one launch, no host read.  Per pair: w = max(x2 - x1, 1), wc = ceil(w) (h likewise;
 *                          sides above MI355DET_KEYPOINT_MAX_SIDE are cut there), torch's bicubic upsample to hc x wc (A = -0.75,
 *                          align_corners False, source (d + 0.5) * (56 / size) - 0.5, tap indices clamped), arg-max with the lowest
 *                          linear index on ties, x = (x_int + 0.5) * (w / wc) + x1 (y likewise), third column 1, score = the upsampled
 *                          value there.  The upsampled map is never stored. */
#define MI355DET_KEYPOINT_MAX_SIDE 4096
int mi355det_flip_resize_keypoints(const float* keypoints, float* out, int64_t g, int32_t num_keypoints, const int64_t* kp_offsets,
                                   const mi355det_ingest_image* table, const mi355det_ingest_image* table_dev, int32_t n, void* stream);
int mi355det_keypoint_targets(const float* keypoints, const int64_t* kp_offsets, int32_t n_images, const float* rois,
                              const int64_t* gt_index, int32_t rows, int32_t valid_rows, int32_t num_keypoints, int32_t heatmap_size,
                              int32_t* target, int32_t* valid, int32_t* count, void* stream);
int mi355det_keypoint_heatmaps(const float* logits, int32_t logits_ld, int32_t padded_keypoints, int32_t rows, int32_t num_keypoints,
                               float* out, void* stream);
size_t mi355det_keypoint_loss_workspace(int32_t rows, int32_t num_keypoints);
int mi355det_keypoint_loss(const float* logits, int32_t logits_ld, int32_t padded_keypoints, int32_t rows, int32_t num_keypoints,
                           const int32_t* target, const int32_t* valid, const int32_t* count, float* loss, void* dlogits,
                           float* dlogits_f32, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int mi355det_heatmaps_to_keypoints(const float* maps, const float* rois, int32_t roi_ld, int32_t rows, int32_t num_keypoints, float* xy,
                                   float* scores, void* stream);

/* ---- Run lengths from counts strings (csrc/rle_string_kernels.hip): mi355det_rle_from_string for the n masks of a results file at once,
 * with the checks, the area and the tight box that the evaluators need of every mask.  bytes: all strings back to back, no separators,
 * num_bytes in all, ON THE DEVICE.  str_offsets int64 [n + 1]: mask k owns bytes[str_offsets[k]:str_offsets[k + 1]]; the same table is
 * read by the host checks (`str_offsets`, host memory) and by the kernels (`str_offsets_dev`, the caller's device copy of it).  sizes int32
 * [n, 2] = [h, w] per mask on the device.  The rules (rleFrString, then the mask store's checks, then rleArea / rleToBbox):
 *   character  c = byte - 48 must lie in 0..63; its low five bits are payload, low group first; bit 0x20: the token goes on.
 *   token      at most 7 characters; bit 0x10 of its last character sign-extends it; the string must end with a finished token.
 *   counts     count m = token m, plus count m - 2 when m > 2: counts 0, 1 and 2 are raw, then two interleaved running sums, one over the
 *              odd indices from 1 and one over the even indices from 2.  Every count must fit int32 and be >= 0, and the counts must add
 *              up to h*w; 1 <= h, w and h*w < 2^31.
 *   area       the sum of the odd-indexed counts.  bbox [xmin, ymin, xmax - xmin + 1, ymax - ymin + 1] over the non-empty runs of ones
 *              (pixels in column-major order i = x*h + y); a run that goes on into the next column spans y = 0..h-1; zeros for an empty
 *              mask.
 * A kernel reads only inside str_offsets_dev[k]:str_offsets_dev[k + 1], whatever the bytes are: a token cut off at the end of its string
 * is a status, and a range that does not lie in [0, num_bytes] (or holds more than 2^28 characters) is skipped with a status.  Malformed
 * input sets the mask's status bits (MI355DET_RLESTR_*, 0 = a valid mask) and nothing else.
 *   rle_strings_count  decodes and checks every mask: status uint8 [n], run_offsets int64 [n + 1] (as mi355det_mask_rle_count gives them:
 *                      run_offsets[k] = index of mask k's first count; a skipped mask has none) and num_bad int64 [1] = the number of masks
 *                      with a status, all on the device; a caller that places num_bad behind run_offsets reads both with one copy.
 *                      EINVAL before any launch for n < 0, a null table, or host str_offsets that do not rise from 0 to num_bytes.
 *   rle_strings_emit   decodes again and writes counts int32 [run_offsets[n]], area int64 [n] and bbox int32 [n, 4] (nullable).  total_runs
 *                      is the caller's host copy of run_offsets[n]; capacity < total_runs is an error and no count is written at an index
 *                      >= capacity or outside the mask's own slots.  What a mask with a status gets is unspecified.
 * Integers only, no atomics, one writer per element: the output is bit-identical from run to run.  No workspace. */
#define MI355DET_RLESTR_RANGE 1     /* the byte range does not fit the buffer: skipped */
#define MI355DET_RLESTR_SIZE 2      /* h, w < 1 or h*w >= 2^31: skipped */
#define MI355DET_RLESTR_ALPHABET 4  /* a character outside the alphabet */
#define MI355DET_RLESTR_LONG 8      /* a token of more than 7 characters */
#define MI355DET_RLESTR_OPEN 16     /* the string ends inside a token */
#define MI355DET_RLESTR_INT32 32    /* a count that does not fit int32 */
#define MI355DET_RLESTR_NEGATIVE 64 /* a negative count */
#define MI355DET_RLESTR_SUM 128     /* the counts do not add up to h*w */
int mi355det_rle_strings_count(const uint8_t* bytes, int64_t num_bytes, const int64_t* str_offsets, const int64_t* str_offsets_dev,
                               const int32_t* sizes, int64_t n, int64_t* run_offsets, uint8_t* status, int64_t* num_bad, void* stream);
int mi355det_rle_strings_emit(const uint8_t* bytes, int64_t num_bytes, const int64_t* str_offsets_dev, const int32_t* sizes, int64_t n,
                              const int64_t* run_offsets, int64_t total_runs, int32_t* counts, int64_t capacity, int64_t* area,
                              int32_t* bbox, void* stream);

/* ---- Mask boundaries as run lengths (csrc/boundary_kernels.hip): the masks that `iou_type="boundary"` of lvis-api and of the COCO
 * boundary-IoU API (Cheng et al., "Boundary IoU", CVPR 2021) compare, made from the masks' run lengths without a bitmap on the host.  The rule:
 *   dilation   d = int(round(ratio * sqrt(h*h + w*w))) in float64 with ties to even, ratio = 0.02 unless given, 1 where that is below 1.  The
 *              caller works it out on the host (rle.boundary_dilation) and hands it in per mask.
 *   erosion    eroded(x, y) = 1 iff the whole (2d+1) x (2d+1) window centred on (x, y) lies inside the image and every pixel of it is set:
 *              copyMakeBorder(1 px of 0) + cv2.erode(3x3 ones, iterations = d) + crop.
 *   boundary   mask & ~eroded: a subset of the mask, hence of the mask's tight box.
 * Boundary IoU is maskUtils.iou (mi355det_coco_iou, run-length mode) on two boundaries with the same iscrowd flags, and the IoU a matcher
 * sees is min(mask IoU, boundary IoU); both are the callers' business (ops.coco_boundary_iou, COCOEval / LVISSegmEval with "boundary").
 * Operands: counts int32 [num_counts] and runs int64 [num_src + 1] as the run-length entries give them (mask s owns counts[runs[s]:
 * runs[s + 1]], which must add up to its h*w; otherwise the result is unspecified, nothing outside the mask's own slots is read or written);
 * index int64 [n] or null: output mask k is the boundary of source mask index[k] (null: of mask k, and num_src >= n); geom int32 [n, 7] =
 * h, w, d, then the mask's tight box x, y, w, h (any box that holds every set pixel gives the same result; w or h of 0: the empty mask);
 * slices int64 [n]: the byte offset of mask k's scratch slice in the workspace.  runs, index, geom and slices are read by the host checks
 * (host memory) and by the kernels (`*_dev`, the caller's device copies), as str_offsets is in mi355det_rle_strings_count.
 *   rle_boundary_plan   host only: checks every mask, lays the slices out in chunks of consecutive masks whose slices together stay within
 *                       budget_bytes (a chunk holds one mask at least) and returns the number of chunks C; chunk_starts int64 [C + 1] (room
 *                       for n + 1) and workspace_bytes [1] = the largest chunk.  A slice holds three bit planes of the box (64 rows a word)
 *                       and the mask's scanned counts.
 *   rle_boundary_count  masks first .. first + num - 1 (one chunk of the plan): num_runs int64 [n] on the device gets each mask's number of
 *                       counts.  The caller's exclusive sum over all n is run_offsets [n + 1]; one host read of it sizes the counts.
 *   rle_boundary_emit   the same chunk again: counts int32 at run_offsets[k], area int64 [n] and bbox int32 [n, 4] (nullable; pycocotools
 *                       `area` / `toBbox` of the boundary).  total_runs is the host copy of run_offsets[n]; capacity < total_runs is an error
 *                       and no count is written at an index >= capacity or outside the mask's own slots.
 * Every entry refuses with EINVAL, before any launch: n < 0, a null table, h or w < 1 or h*w >= 2^31, d < 1, a box that leaves its image, an
 * index that is no source mask, runs that leave the counts; EWORKSPACE: slices that overlap or leave the workspace.  Chunks of one plan may
 * share one workspace on one stream.  Integers only, no atomics, one writer per element: the output is bit-identical from run to run and does
 * not depend on the chunking. */
int64_t mi355det_rle_boundary_plan(const int64_t* runs, int64_t num_src, int64_t num_counts, const int64_t* index, const int32_t* geom, int64_t n,
                                   int64_t budget_bytes, int64_t* slices, int64_t* chunk_starts, int64_t* workspace_bytes);
int mi355det_rle_boundary_count(const int32_t* counts, int64_t num_counts, const int64_t* runs, const int64_t* runs_dev, int64_t num_src,
                                const int64_t* index, const int64_t* index_dev, const int32_t* geom, const int32_t* geom_dev,
                                const int64_t* slices, const int64_t* slices_dev, int64_t n, int64_t first, int64_t num, int64_t* num_runs,
                                void* workspace, size_t workspace_bytes, void* stream);
int mi355det_rle_boundary_emit(const int32_t* counts, int64_t num_counts, const int64_t* runs, const int64_t* runs_dev, int64_t num_src,
                               const int64_t* index, const int64_t* index_dev, const int32_t* geom, const int32_t* geom_dev,
                               const int64_t* slices, const int64_t* slices_dev, int64_t n, int64_t first, int64_t num,
                               const int64_t* run_offsets, int64_t total_runs, int32_t* out_counts, int64_t capacity, int64_t* area,
                               int32_t* bbox, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Polygon ground truth as COCO run-length encodings (csrc/poly_kernels.hip; torchvision_models/detection/coco_utils.py:33-47
 * convert_coco_poly_to_mask = pycocotools frPyObjects + decode + any over the parts).  One polygon is k >= 3 points xy (float64, x then y);
 * its annotation's image is h x w.  The rules of pycocotools rleFrPoly, then rleMerge as a union:
 *   scale     X[j] = (int)(5*x[j] + .5), Y[j] likewise (the C cast: truncation toward zero, also for negatives); X[k] = X[0] closes the ring.
 *   walk      every edge j -> j+1: dx = |xe-xs|, dy = |ye-ys|, flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye), the end points swapped
 *             when flipped, s = dx >= dy ? (double)(ye-ys)/dx : (double)(xe-xs)/dy.  dx >= dy: for d = 0..dx, t = flip ? dx-d : d,
 *             u = t + xs, v = (int)(ys + s*t + .5).  Otherwise for d = 0..dy, t = flip ? dy-d : d, v = t + ys, u = (int)(xs + s*t + .5).
 *             The edges' points one after the other; a zero-length edge gives its one point.
 *   points    each consecutive pair with u[j] != u[j-1]: xd = u[j] < u[j-1] ? u[j] : u[j]-1, xd = (xd+.5)/5 - .5, dropped unless
 *             floor(xd) == xd and 0 <= xd <= w-1; yd = min(v[j], v[j-1]), yd = (yd+.5)/5 - .5, clamped to [0, h], then ceil;
 *             a = (int)xd*h + (int)yd.
 *   runs      h*w appended, sorted, differences (the first from 0): the first difference is the first count, a positive one the next count,
 *             a zero one is skipped and the difference after it added to the last count.  Equivalently the run boundaries are the
 *             positions below h*w that occur an odd number of times, which is what the kernels use.
 *   union     an annotation's mask is the union of its parts' masks, canonical (no zero count except possibly the first); without parts
 *             it is the all-zero mask [h*w].
 * All arithmetic is float64 without contraction, divisions IEEE.  The caller validates the input (finite coordinates, |c| < 2^24, k >= 3,
 * h, w >= 1, h*w < 2^31, rising offsets): the kernels only promise to write nothing outside the stated capacities.
 * Tables ON THE DEVICE: xy float64 [2 * points]; poly_offsets int64 [num_polys + 1] in points; ann_offsets int64 [num_anns + 1] in polygons
 * (annotation a owns the polygons ann_offsets[a]..ann_offsets[a + 1]); sizes int32 [num_anns, 2] = [h, w], which may differ between
 * annotations.
 *   poly_points_count  point_offsets int64 [num_polys + 1]: the index of polygon p's first kept point, [num_polys] = their number.
 *   poly_points_emit   keys int64 [total_points] = polygon index << 32 | a, each polygon's in its slots in a fixed order.  total_points is
 *                      the caller's host copy of point_offsets[num_polys].  THE CALLER SORTS the keys ascending before the passes below.
 *   poly_events        for every polygon of an annotation with two or more parts: its r-th run boundary (rising) as the event
 *                      annotation << 32 | position << 1 | (r & 1) at events[event_base[p] + r]; the rest of the polygon's
 *                      point_offsets[p + 1] - point_offsets[p] slots is filled with INT64_MAX.  event_base int64 [num_polys] (the caller's
 *                      exclusive sum of the point counts of such polygons; < 0 = skip).  toggle_offsets int64 [num_polys + 1]: the
 *                      exclusive sum of the events per polygon.  THE CALLER SORTS events ascending.
 *   poly_runs_count    run_offsets int64 [num_anns + 1], as mi355det_mask_rle_count gives them.
 *   poly_runs_emit     counts int32 [run_offsets[num_anns]], area int64 [num_anns] and bbox int32 [num_anns, 4] (nullable) as
 *                      mi355det_mask_rle_emit gives them; a run of ones that goes on into the next column makes the box span y = 0..h-1.
 *                      capacity < total_runs is an error and no count is written at an index >= capacity.
 *   rle_decode         counts + run_offsets [num_masks + 1] (ON THE DEVICE) of masks of one size -> uint8 [num_masks, im_h, im_w] row-major,
 *                      1 inside the odd-indexed runs; counts past im_h*im_w are cut there.
 * No atomics; every output is bit-identical from run to run.  No entry point needs a workspace. */
int mi355det_poly_points_count(const double* xy, const int64_t* poly_offsets, const int64_t* ann_offsets, const int32_t* sizes,
                               int32_t num_polys, int32_t num_anns, int64_t* point_offsets, void* stream);
int mi355det_poly_points_emit(const double* xy, const int64_t* poly_offsets, const int64_t* ann_offsets, const int32_t* sizes,
                              int32_t num_polys, int32_t num_anns, const int64_t* point_offsets, int64_t total_points, int64_t* keys,
                              int64_t capacity, void* stream);
int mi355det_poly_events(const int64_t* keys, const int64_t* point_offsets, const int64_t* ann_offsets, const int32_t* sizes,
                         const int64_t* event_base, int32_t num_polys, int32_t num_anns, int64_t* events, int64_t capacity,
                         int64_t* toggle_offsets, void* stream);
int mi355det_poly_runs_count(const int64_t* keys, const int64_t* point_offsets, const int64_t* events, const int64_t* toggle_offsets,
                             const int64_t* ann_offsets, const int32_t* sizes, int32_t num_polys, int32_t num_anns, int64_t* run_offsets,
                             void* stream);
int mi355det_poly_runs_emit(const int64_t* keys, const int64_t* point_offsets, const int64_t* events, const int64_t* toggle_offsets,
                            const int64_t* ann_offsets, const int32_t* sizes, int32_t num_polys, int32_t num_anns, const int64_t* run_offsets,
                            int64_t total_runs, int32_t* counts, int64_t capacity, int64_t* area, int32_t* bbox, void* stream);
int mi355det_rle_decode(const int32_t* counts, const int64_t* run_offsets, int32_t num_masks, int32_t im_h, int32_t im_w, uint8_t* out,
                        void* stream);

/* ---- COCO evaluation (csrc/cocoeval_kernels.hip): pycocotools maskUtils.iou, COCOeval.evaluateImg and COCOeval.accumulate for `bbox` and
 * `segm`.  A group is one (image, category) pair: D detections in descending score order (stable, cut to the largest maxDets by the caller)
 * and G ground truths in annotation order.  dt_offsets / gt_offsets / iou_offsets [num_groups + 1] int64 ON THE DEVICE: group j owns the
 * detection slots dt_offsets[j]..dt_offsets[j + 1], the ground-truth slots likewise and the row-major [D, G] float64 matrix at
 * iou[iou_offsets[j]].  num_dt / num_gt / iou_size are the caller's host copies of the last offsets: they size every array below, and a
 * group that does not fit them is skipped, never written past.  All floating point is float64 without contraction; no atomics, every output
 * element has one writer, so the output is bit-identical from run to run.  No entry point needs a workspace; each validates its arguments
 * on the host and returns without a launch when there are no groups (categories).
 *   coco_iou         boxes [x, y, w, h] float64: da = dw*dh, ga = gw*gh, w = min(dx+dw, gx+gw) - max(dx, gx) (<= 0: IoU 0), h likewise,
 *                    i = w*h, u = gt_crowd ? da : da + ga - i, iou = i/u.  rle_mode = 0: dt_boxes [num_dt, 4], gt_boxes [num_gt, 4] are the
 *                    boxes.  rle_mode = 1: they are the masks' tight boxes (toBbox, zeros for an empty mask) and reject first (box IoU 0 ->
 *                    0); otherwise one lane walks both run lists (mi355det_mask_rle_* format: column-major, a zero run first) and counts
 *                    i and both areas; i == 0 -> 0, else the same i/u.  The run lists are counts + runs [masks + 1] as RLEBatch holds
 *                    them; index (nullable = identity) maps a slot to its mask.  dt_sizes / gt_sizes are HOST arrays [num_groups, 2] of
 *                    [h, w], [0, 0] for a side without masks: differing sizes within a group are MI355DET_EINVAL before any launch.
 *   coco_match       lane a*num_thrs + t of the group's wavefront runs the greedy match of area range a at IoU threshold t (num_areas *
 *                    num_thrs <= 64).  iou_thrs [num_thrs], area_rngs [num_areas, 2] float64 on the device, built by the caller (never
 *                    recomputed here).  gt_ignore [num_areas, num_gt] uint8 = crowd, or area outside the range.  Per detection in score
 *                    order: best = min(thr, 1 - 1e-10); walk the non-ignored ground truths, then (only while unmatched) the ignored
 *                    ones, each in annotation order; skip one already matched unless crowd; skip iou < best (strict); else take it.
 *                    dt_match [num_areas, num_thrs, num_dt] int32 = 0 or the ground truth's index in its group + 1; gt_match [num_areas,
 *                    num_thrs, num_gt] int32 = 0 or the detection's index in its group + 1; dt_ignore [num_areas, num_thrs, num_dt] uint8 =
 *                    the matched ground truth's flag, or for an unmatched detection dt_area outside the range.
 *   lvis_match       coco_match under the rules of lvis-api's LVISEval (same kernel body, same outputs and layouts, same guarantees).  LVIS
 *                    has no crowds: gt_flag [num_gt] uint8 is the annotation's `ignore` flag, gt_ignore = gt_flag, or area outside the
 *                    range, and a ground truth already matched at this threshold is always skipped (no re-match).
 *                    group_not_exhaustive [num_groups] uint8 ON THE DEVICE: the group's category is in its image's
 *                    not_exhaustive_category_ids; dt_ignore of an unmatched detection = dt_area outside the range, or that flag.  A missing
 *                    group_not_exhaustive with num_groups > 0 is MI355DET_EINVAL.  The IoU comes from coco_iou with an all-zero gt_crowd
 *                    (never the ignore flags); coco_accumulate takes the outputs as they are, with one max_dets that cuts nothing.
 *   coco_accumulate  the slots are category-major: category k owns cat_dt_offsets[k]..[k + 1] and cat_gt_offsets[k]..[k + 1] (int64
 *                    [num_cats + 1] on the device).  order [num_dt] int64: per category its slots in descending score order (stable);
 *                    dt_rank [num_dt] int32: the slot's rank within its group; max_dets is a HOST array (at most 8).  Per (k, a, m, t):
 *                    detections with rank < max_dets[m] in `order`; npig = non-ignored ground truths; tp / fp cumulative sums; rc =
 *                    tp/npig; pr = tp/(fp + tp + 2^-52) made non-increasing from the right; recall [num_thrs, K, A, M] = the last rc (0
 *                    without detections); precision / scores [num_thrs, num_recs, K, A, M] = pr / score at the first index with rc >=
 *                    rec_thrs[r] (float64 on the device), 0 past the end; everything -1 where npig == 0. */
int mi355det_coco_iou(int32_t rle_mode, int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets,
                      int64_t num_dt, int64_t num_gt, int64_t iou_size, const double* dt_boxes, const double* gt_boxes, const uint8_t* gt_crowd,
                      const int32_t* dt_counts, const int64_t* dt_runs, const int64_t* dt_index, int64_t dt_masks, int64_t dt_num_counts,
                      const int32_t* gt_counts, const int64_t* gt_runs, const int64_t* gt_index, int64_t gt_masks, int64_t gt_num_counts,
                      const int32_t* dt_sizes, const int32_t* gt_sizes, double* iou, void* stream);
int mi355det_coco_match(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                        int64_t num_gt, int64_t iou_size, const double* iou, const double* dt_area, const double* gt_area,
                        const uint8_t* gt_crowd, const double* iou_thrs, int32_t num_thrs, const double* area_rngs, int32_t num_areas,
                        int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, void* stream);
int mi355det_lvis_match(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                        int64_t num_gt, int64_t iou_size, const double* iou, const double* dt_area, const double* gt_area,
                        const uint8_t* gt_flag, const uint8_t* group_not_exhaustive, const double* iou_thrs, int32_t num_thrs,
                        const double* area_rngs, int32_t num_areas, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore,
                        void* stream);
int mi355det_coco_accumulate(int32_t num_cats, const int64_t* cat_dt_offsets, const int64_t* cat_gt_offsets, int64_t num_dt, int64_t num_gt,
                             const int64_t* order, const int32_t* dt_rank, const double* dt_score, const int32_t* dt_match,
                             const uint8_t* dt_ignore, const uint8_t* gt_ignore, int32_t num_thrs, int32_t num_areas, const int32_t* max_dets,
                             int32_t num_max_dets, const double* rec_thrs, int32_t num_recs, double* precision, double* recall, double* scores,
                             void* stream);

/* ---- COCO keypoint evaluation (csrc/oks_kernels.hip, csrc/cocoeval_kernels.hip): pycocotools COCOeval.computeOks and evaluateImg for
 * `keypoints`, on the groups, offsets and guarantees of the "COCO evaluation" block above.  pycocotools is not installed where this was
 * written: the rules below are restated from memory of its cocoeval.py, and the tests compare against a literal host form of this text.
 *   coco_oks         the ragged buffer of coco_iou (same offsets, one wavefront per group, row-major [D, G] per group, float64) filled with
 *                    the object keypoint similarity.  Operands ON THE DEVICE, K = num_keypoints per instance: dt_kp float64 [num_dt, K, 2] =
 *                    x, y of each keypoint (a detection's visibility is never read); gt_kp float64 [num_gt, K, 3] = x, y, v; gt_boxes
 *                    float64 [num_gt, 4] = [x, y, w, h]; gt_area float64 [num_gt]; vars float64 [K] = (2 * sigma)^2, built by the caller
 *                    (never recomputed here).  Per ground truth: k1 = the number of keypoints with v > 0; x0 = bx - bw, x1 = bx + bw*2,
 *                    y0 = by - bh, y1 = by + bh*2.  Per pair and keypoint i: if k1 > 0, dx = xd - xg, dy = yd - yg; else dx = max(0, x0 -
 *                    xd) + max(0, xd - x1) and dy likewise; e = (dx*dx + dy*dy) / vars[i] / (area + 2^-52) / 2, left to right.  oks =
 *                    sum(exp(-e_i)) / n over the keypoints with v > 0, n = k1, when k1 > 0; over all K keypoints, n = K, otherwise.  The
 *                    sum runs in ascending keypoint order in one lane (the order is part of the contract); exp is the device library's
 *                    float64 exp; the ground truths of a group are staged in LDS once per group.  Crowd plays no part.
 *                    MI355DET_EINVAL before any launch: num_keypoints < 1 or > 64, negative sizes, a missing operand with groups present.
 *   keypoints_match  coco_match with the two ground-truth flags apart (same kernel body through one more template switch; same outputs,
 *                    layouts, guarantees and 64-lane limit).  gt_flag [num_gt] uint8 = the annotation's ignore flag (iscrowd, or
 *                    num_keypoints == 0); gt_crowd [num_gt] uint8 = iscrowd alone.  gt_ignore = gt_flag, or area outside the range; a
 *                    ground truth already matched at this threshold is skipped unless gt_crowd is set. */
int mi355det_coco_oks(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                      int64_t num_gt, int64_t iou_size, int32_t num_keypoints, const double* dt_kp, const double* gt_kp,
                      const double* gt_boxes, const double* gt_area, const double* vars, double* oks, void* stream);
int mi355det_keypoints_match(int64_t num_groups, const int64_t* dt_offsets, const int64_t* gt_offsets, const int64_t* iou_offsets, int64_t num_dt,
                             int64_t num_gt, int64_t iou_size, const double* iou, const double* dt_area, const double* gt_area,
                             const uint8_t* gt_flag, const uint8_t* gt_crowd, const double* iou_thrs, int32_t num_thrs, const double* area_rngs,
                             int32_t num_areas, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, void* stream);

/* ---- Bootstrap replicates (csrc/bootstrap_kernels.hip): coco_accumulate for num_replicates resampled data sets at once, reduced in place to
 * one precision sum and one recall per cell.  The arguments of coco_accumulate without the scores (same layouts, same meaning; the match
 * arrays are those of coco_match / lvis_match and are not touched), plus dt_image [num_dt] / gt_image [num_gt] int32 = each slot's image
 * index and weights [num_images, num_replicates] int32 ON THE DEVICE, replicate-minor.
 *   replicate b      the data set in which image i occurs weights[i][b] times, copies adjacent in image order.  Matching is per (image,
 *                    category) group and does not change; only the accumulate pass does.
 *   per (b, k, a, m, t)   npig = sum of weights[gt_image][b] over the category's non-ignored ground truths.  The kept detections (rank <
 *                    max_dets[m]) of weight > 0 in `order`; tp and fp advance by the weight per slot; at the end of each slot rc = tp/npig
 *                    and pr = tp/(fp + tp + 2^-52), the expressions of coco_accumulate; pr made non-increasing from the right; recall
 *                    threshold r takes pr at the first slot with rc >= rec_thrs[r], 0 past the end.  The first kept slot owns threshold 0
 *                    whatever its flags.  (This is the replicated data set exactly unless two kept detections of ONE group have equal
 *                    scores and different flags: the replicated set interleaves their copies, this rule keeps each slot's copies adjacent.)
 *   outputs          ap_sum, recall float64 [num_replicates, num_thrs, K, A, M].  ap_sum = the sum of the cell's num_recs precision values,
 *                    added one by one in float64 in order of DESCENDING recall threshold (never count * value; an unreached threshold adds
 *                    0.0); recall = total tp / npig, 0 without kept detections; both -1.0 where npig == 0.
 * A slot whose image index lies outside [0, num_images) has weight 0 and no weight is read for it; a negative weight counts as 0.
 * float64 without contraction, no atomics, one writer per element, 64-bit offsets: bit-identical from run to run and whatever the number of
 * replicates per call.  No workspace.  MI355DET_EINVAL: a missing operand; num_cats, num_thrs, num_areas, num_max_dets, num_recs, num_images
 * or num_replicates <= 0; num_dt or num_gt < 0; num_recs > 4096; num_max_dets > 8. */
int mi355det_coco_bootstrap(int32_t num_cats, const int64_t* cat_dt_offsets, const int64_t* cat_gt_offsets, int64_t num_dt, int64_t num_gt,
                            const int64_t* order, const int32_t* dt_rank, const int32_t* dt_match, const uint8_t* dt_ignore,
                            const uint8_t* gt_ignore, int32_t num_thrs, int32_t num_areas, const int32_t* max_dets, int32_t num_max_dets,
                            const double* rec_thrs, int32_t num_recs, const int32_t* dt_image, const int32_t* gt_image, const int32_t* weights,
                            int32_t num_images, int32_t num_replicates, double* ap_sum, double* recall, void* stream);

/* ---- Dataset statistics (csrc/dstats_kernels.hip): the per-class table that parameterises TF-IDF re-weighting, from the annotations - what
 * the reference's yolo/utilities/get_idf.py and IDFTransformer's build branch (custom.py:176-247) compute image by image on the host.
 *   category_frequencies   image_index, category_index int32 [n_annotations] ON THE DEVICE, one pair per annotation ->
 *                    instance_freq[c] = the number of annotations of category c, img_freq[c] = the number of distinct images with at least
 *                    one annotation of c; both int32 [n_categories].  Integer atomics only: exact, independent of the order of the
 *                    annotations and of scheduling, bit-identical from run to run.  Distinct (image, category) pairs are found with a bitmap
 *                    of n_images x ceil(n_categories / 32) 32-bit words = the workspace (category_frequencies_workspace bytes); the call
 *                    zeroes the bitmap, both outputs and `errors` on the stream.  A pair whose image index lies outside [0, n_images) or
 *                    whose category index lies outside [0, n_categories) is not counted and touches no memory; it adds 1 to errors[0]
 *                    (int32 on the device), which the caller reads.  Up to category_frequencies_lds_categories() categories the two
 *                    histograms are kept per workgroup in LDS and only non-zero bins reach memory; beyond, global atomics.
 *   idf_table        img_freq, instance_freq int32 [n_rows] (the categories that occur: both > 0), n_images = D -> table float64
 *                    [14, n_rows], rows in this order: smooth, raw, prob, normit, gombit, base2, base10, then the same seven `_obj`.
 *                    With df = img_freq, p = df / D:  smooth = log((D + 1) / (df + 1)) + 1, raw = log(D / df), prob = log((D - df) / df),
 *                    normit = -ndtri(p), gombit = -log(-log(1 - p)), base2 = -log2(p), base10 = -log10(p); the `_obj` rows with
 *                    N = sum of instance_freq (summed in integers) for D and instance_freq for df.  ndtri = the inverse normal
 *                    distribution function by Cephes' rational approximations (scipy.special.ndtri).  float64 without contraction, one
 *                    writer per element.  p = 1 (a category in every image, or a single category) gives prob = normit = gombit = -inf
 *                    as numpy does, never NaN.
 * MI355DET_EINVAL: a missing operand; n_images, n_categories or n_rows <= 0; n_annotations < 0 or >= 2^31; a workspace that is too small. */
size_t mi355det_category_frequencies_workspace(int32_t n_images, int32_t n_categories);
int mi355det_category_frequencies_lds_categories(void);
int mi355det_category_frequencies(const int32_t* image_index, const int32_t* category_index, int64_t n_annotations, int32_t n_images,
                                  int32_t n_categories, int32_t* instance_freq, int32_t* img_freq, int32_t* errors, void* workspace,
                                  size_t workspace_bytes, void* stream);
int mi355det_idf_table(const int32_t* img_freq, const int32_t* instance_freq, int32_t n_rows, int64_t n_images, double* table, void* stream);

/* ---- Anchor k-means (csrc/kmeans_kernels.hip): the anchor list of a dataset from its annotations - what the reference's
 * yolo/utilities/kmeans_anchors.py computes with pandas and scikit-learn (the first three anchors per scale of yolo/hydra/dataset/lvis.yaml) -
 * and k-means on (w, h) under the 1 - IoU distance.  All arithmetic is float64 IEEE without contraction; no floating-point atomics.
 *   features         per annotation of a listed image (kmeans_anchors.py:20-49), in this order: width = bbox[2] / W, height = bbox[3] / H,
 *                    aspect = width / height, area = width * height, with W, H the image's integer sizes converted to float64.
 *   selection, bands a box is kept iff aspect > 0.2 && aspect < 5 (strict; NaN and infinity from a zero height or size fall out by
 *                    themselves).  Band 0 (small): area < 0.01; band 1 (medium): area > 0.01 && area < 0.1; band 2 (large): area > 0.1.  A
 *                    kept box whose area is exactly 0.01 or 0.1 belongs to no band, as in the script; it and every dropped box have band -1.
 *   distance         MI355DET_KMEANS_EUCLID: ((x0 - c0)^2 + (x1 - c1)^2) + ..., summed in feature order.  MI355DET_KMEANS_IOU (features = 2,
 *                    x = (w, h)): 1 - i / (w * h + cw * ch - i) with i = min(w, cw) * min(h, ch).
 *   Lloyd pass       for one problem (the points of one band, or all points) and one restart: every point goes to the centre with the
 *                    smallest distance, ties to the lowest centre index.  After a pass every non-empty cluster's centre becomes
 *                    sum / count; an EMPTY cluster keeps its centre (scikit-learn relocates it: a stated deviation).  Iteration stops after
 *                    the first pass in which no label changed - the first pass always counts as changed - or after max_iter passes.  The
 *                    result is the centres the last assignment was made against, that assignment's labels and counts, and the inertia =
 *                    the sum of the minimal distances of that pass.  Restarts differ in their initial centres only; the caller picks the
 *                    lowest inertia, ties to the lowest restart.
 *   sums             a workgroup owns kmeans_limit(5) = 256 consecutive points.  Per (problem, restart, cluster) and feature it adds the
 *                    points of that cluster, and per (problem, restart) the minimal distances of all the problem's points (the inertia),
 *                    in ascending point order; the partials of workgroups l, l + 64, ... are added in ascending order by lane l of one
 *                    wave, and the 64 lane sums are folded by a fixed xor butterfly (offsets 32, 16, ... 1).  So the order of every sum
 *                    depends on n and the point's places alone, results are bit-identical from run to run, and two restarts that end in
 *                    the same clustering with the clusters numbered differently have the same inertia bits (a tie, so the lower restart
 *                    wins).  Counts and changed-label counts are integers (atomics).
 * box_features       box_wh float64 [n_annotations, 2] = (bbox[2], bbox[3]), image_index int32 [n_annotations], image_size int32
 *                    [n_images, 2] = (W, H) -> features float64 [n_annotations, 4], band int8 [n_annotations].  An image index outside
 *                    [0, n_images) adds 1 to errors[0] (int32 on the device, zeroed by the call) and gives NaN features and band -1.
 * kmeans_check       errors[0] = points with problem >= 0 that have a non-finite feature or, with the IoU distance, a non-positive one;
 *                    errors[1] = points with problem >= problems.  int32 [2] on the device, zeroed by the call.
 * kmeans_begin       resets a run: the previous labels (so that the first pass counts as changed), the done flags, status[0] and n_iter.
 * kmeans_passes      enqueues n_passes Lloyd passes (two launches each, no host synchronisation) over x float64 [n, features] for all
 *                    problems and restarts at once: problem int8 [n] gives each point's problem (NULL: all 0; < 0 or >= problems: the point
 *                    takes part in nothing).  centers float64 [problems, restarts, k, features] in and out; per pass of an unfinished
 *                    (problem, restart) the call writes sums [problems, restarts, k, features], counts int32 [problems, restarts, k],
 *                    inertia float64 [problems, restarts], changed int32 [problems, restarts] and adds 1 to n_iter int32
 *                    [problems, restarts].  A finished (problem, restart) is frozen; status[0] counts them, and passes enqueued after
 *                    status[0] = problems * restarts return at once.  The caller reads status[0] every few passes.
 * kmeans_assign      labels int32 [n] and the minimal distance float64 [n] against centers [problems, k, features] (k up to
 *                    kmeans_limit(4)); a point that takes part in nothing gets label -1 and distance 0.
 * kmeans_limit       0: problems <= 4, 1: restarts <= 16, 2: k <= 16, 3: features <= 4, 4: k of kmeans_assign <= 64, 5: points per workgroup.
 * MI355DET_EINVAL: a missing operand; n <= 0 or >= 2^31; a size <= 0 or beyond its limit; the IoU distance with features != 2;
 * max_iter or n_passes <= 0; a workspace smaller than kmeans_workspace (which is 0 for sizes it refuses). */
#define MI355DET_KMEANS_EUCLID 0
#define MI355DET_KMEANS_IOU 1
int mi355det_kmeans_limit(int which);
int mi355det_box_features(const double* box_wh, const int32_t* image_index, const int32_t* image_size, int64_t n_annotations, int32_t n_images,
                          double* features, int8_t* band, int32_t* errors, void* stream);
size_t mi355det_kmeans_workspace(int64_t n, int32_t problems, int32_t restarts, int32_t k, int32_t features);
int mi355det_kmeans_check(const double* x, const int8_t* problem, int64_t n, int32_t problems, int32_t features, int32_t metric, int32_t* errors,
                          void* stream);
int mi355det_kmeans_begin(int64_t n, int32_t problems, int32_t restarts, int32_t k, int32_t features, int32_t* n_iter, int32_t* status,
                          void* workspace, size_t workspace_bytes, void* stream);
int mi355det_kmeans_passes(const double* x, const int8_t* problem, int64_t n, int32_t problems, int32_t restarts, int32_t k, int32_t features,
                           int32_t metric, int32_t max_iter, int32_t n_passes, double* centers, double* sums, int32_t* counts, double* inertia,
                           int32_t* n_iter, int32_t* changed, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int mi355det_kmeans_assign(const double* x, const int8_t* problem, int64_t n, int32_t problems, int32_t k, int32_t features, int32_t metric,
                           const double* centers, int32_t* labels, double* distance, void* stream);

/* ---- Model comparison (csrc/compare_kernels.hip): for two result sets over one ground truth, the best class-agnostic box overlap of every
 * ground-truth instance and whether that detection carries the right label - the per-image body of the reference's
 * notebooks/get_disagreement.py (torchvision box_iou, then max over the detections), for all images and both models in one launch.
 * gt_offsets / dt_offsets_a / dt_offsets_b [num_images + 1] int64 ON THE DEVICE: image i owns the ground-truth slots gt_offsets[i]..
 * gt_offsets[i + 1] and, per model, the detection slots dt_offsets[i]..dt_offsets[i + 1]; gt_offsets must run from 0 to num_gt (a slot no
 * image owns is not written).  num_gt / num_dt_a / num_dt_b are the caller's host copies of the last offsets: they size the arrays, an
 * image whose ground-truth range does not fit is skipped and one whose detection range does not fit (or holds more than 2^31 - 1
 * detections: best_index is int32) counts as having no detections; nothing is read or written past them.  Boxes are float64 [*, 4] as
 * [x, y, w, h] with finite entries, labels int64.  Outputs [2, num_gt], model a first: best_iou float64, best_index int32 (the detection's
 * index within its image), correct uint8.  All floating point is float64 without contraction, the division is IEEE; no atomics, every
 * output element has one writer, so the output is bit-identical from run to run.  No workspace; MI355DET_EINVAL for num_images < 0 and
 * for missing offset tables with num_images > 0; no launch when there are no images or no ground truths.
 *   per box          x2 = x + w, y2 = y + h first; area = (x2 - x) * (y2 - y) (not w * h: they differ in the last bit).
 *   per pair         iw = max(min(dx2, gx2) - max(dx, gx), 0), ih likewise, inter = iw * ih, iou = inter / (da + ga - inter); a pair with
 *                    zero union is 0 / 0 = NaN.
 *   per ground truth the best detection as torch.max(iou, dim=0) picks it: NaN beats every number; among equal values, or among several
 *                    NaNs, the lowest detection index wins.  correct = best_iou >= iou_threshold && gt_label == dt_label[best_index] (a NaN
 *                    best is incorrect).  An image without detections of a model gives best_iou 0, best_index -1, correct 0 and reads
 *                    no box and no label of that model. */
int mi355det_box_disagreement(int64_t num_images, const int64_t* gt_offsets, int64_t num_gt, const double* gt_box, const int64_t* gt_label,
                              const int64_t* dt_offsets_a, int64_t num_dt_a, const double* dt_box_a, const int64_t* dt_label_a,
                              const int64_t* dt_offsets_b, int64_t num_dt_b, const double* dt_box_b, const int64_t* dt_label_b,
                              double iou_threshold, double* best_iou, int32_t* best_index, uint8_t* correct, void* stream);

/* ---- Error breakdown (csrc/tide_kernels.hip): why an evaluated COCOEval / LVISEval (`bbox`) loses AP50, after TIDE (Bolya et al., ECCV
 * 2020).  Every false positive is one of five kinds, the unexplained false negatives are a sixth, and each kind is priced by the AP50 gained
 * when that kind alone is fixed; the pricing itself is mi355det_coco_accumulate on the flag arrays tide_fixes writes.
 * Inputs.  fg = 0.5 must be one of the evaluator's IoU thresholds (index t), bg = 0.1; area range 0 (`all`); the detections are the
 *   evaluator's kept slots.  A detection is a FALSE POSITIVE when dt_match[0, t, d] == 0 && dt_ignore[0, t, d] == 0.  A ground truth is
 *   COUNTED when gt_ignore[0, g] == 0, FREE when counted and gt_match[0, t, g] == 0, USED when counted and matched.  A ground truth that is
 *   not counted (COCO: crowds; LVIS: the ignore flags) takes no part anywhere below.
 * Overlap.  The pair expression of mi355det_coco_iou in its non-crowd form, float64, no contraction, IEEE division: da = dw*dh, ga = gw*gh,
 *   w = min(dx+dw, gx+gw) - max(dx, gx), h likewise; w <= 0 || h <= 0 gives 0, otherwise i = w*h and iou = i/(da + ga - i): for a pair of one
 *   category the bits coco_iou wrote.
 * Per false positive d of image i and category k.  Walk the counted ground truths of image i in ascending slot order: s, gs = the largest
 *   overlap with one of category k and that ground truth; o, go = the same over every other category; strict > updates (the lowest slot wins
 *   a tie); without a candidate the value is 0 and the partner -1.  The first test that holds names the kind:
 *     1 Cls   o >= fg                 partner go        (tested second)
 *     2 Loc   bg <= s < fg            partner gs        (tested first)
 *     3 Both  everything else                           (tested last)
 *     4 Dupe  s >= fg                                   (tested third)
 *     5 Bkg   max(s, o) <= bg                           (tested fourth)
 *   A detection that is not a false positive has kind 0, partner -1 and both overlaps 0.
 * Miss.  A free ground truth that is the partner of no Loc and of no Cls detection, whatever the claims below decide.
 * Fixes, each applied alone to the base state.  Loc: walk the image's Loc detections in claim order (descending score, then ascending
 *   dt_index); one whose partner is free and not yet claimed in this walk claims it and becomes a true positive, every other Loc detection
 *   is dropped.  Cls: the same walk over the Cls detections; a claimant becomes a true positive of the partner's category, the others are
 *   dropped.  Both / Dupe / Bkg: those detections are dropped.  Miss: the missed ground truths stop being counted.  FP: every false
 *   positive is dropped.  FN: every free ground truth stops being counted.
 * Price.  dAP[kind] = AP50(fixed) - AP50(base), AP50 = the mean over the categories with a counted ground truth of the 101 precision values
 *   at threshold t, area `all`, from coco_accumulate with dt_rank zero and one max_dets that cuts nothing.  The eight deltas do not add up
 *   to 1 - AP50: each fix is priced alone.
 * The image-major view (both entries).  img_dt_offsets / img_gt_offsets [num_images + 1] and img_dt_slots [num_dt] / img_gt_slots [num_gt],
 *   int64 ON THE DEVICE: image i owns the entries offsets[i]..offsets[i + 1] of the slot lists; its detection slots stand in claim order, its
 *   ground-truth slots ascending.  num_dt / num_gt are the caller's host copies of the last offsets and size every array: an image whose
 *   ranges do not fit them is skipped, a slot outside them is passed over, nothing is read or written past them.  dt_cat / gt_cat int32 =
 *   each slot's category index; dt_fp, gt_counted, gt_free uint8 = the flags above; boxes float64 [*, 4] as [x, y, w, h].
 *   tide_classify    -> kind uint8 [num_dt], partner int64 [num_dt] (a ground-truth slot or -1), best_same / best_other float64 [num_dt] (s, o),
 *                    missed uint8 [num_gt].
 *   tide_fixes       dt_match int32 [num_dt] / dt_ignore uint8 [num_dt] = the evaluator's rows [0, t].  -> fix_dt_match int32 / fix_dt_ignore
 *                    uint8 [8, 1, num_dt] and fix_gt_ignore uint8 [8, num_gt], the fix in the place of the area range, rows base, Loc,
 *                    Both, Dupe, Bkg, Miss, FP, FN: a dropped detection has dt_ignore 1, a new true positive dt_match 1 and dt_ignore 0,
 *                    an uncounted ground truth gt_ignore 1.  The Cls fix moves detections between categories, so it comes per slot:
 *                    cls_cat int32 (the partner's category for a claimant, else dt_cat), cls_match int32, cls_ignore uint8 [num_dt]; the
 *                    caller sorts the slots by cls_cat and calls coco_accumulate once more.
 * One wavefront per image; all floating point is float64 without contraction; no atomics, every output element has one writer (tide_classify
 * clears a partner's `missed` byte from every lane that names it: the same value), so the output is bit-identical from run to run and the
 * winner of a claim depends on the claim order alone.  No workspace.  Both entries return MI355DET_EINVAL before any launch for a negative
 * size and for a missing operand of a side that has slots, tide_classify also for thresholds outside (0, 1] or fg <= bg (tide_fixes takes no
 * threshold); neither launches when there are no images or no slots at all. */
int mi355det_tide_classify(int64_t num_images, const int64_t* img_dt_offsets, const int64_t* img_dt_slots, int64_t num_dt,
                           const int64_t* img_gt_offsets, const int64_t* img_gt_slots, int64_t num_gt, const double* dt_boxes,
                           const int32_t* dt_cat, const uint8_t* dt_fp, const double* gt_boxes, const int32_t* gt_cat, const uint8_t* gt_counted,
                           const uint8_t* gt_free, double fg, double bg, uint8_t* kind, int64_t* partner, double* best_same, double* best_other,
                           uint8_t* missed, void* stream);
int mi355det_tide_fixes(int64_t num_images, const int64_t* img_dt_offsets, const int64_t* img_dt_slots, int64_t num_dt,
                        const int64_t* img_gt_offsets, const int64_t* img_gt_slots, int64_t num_gt, const int32_t* dt_match,
                        const uint8_t* dt_ignore, const int32_t* dt_cat, const int32_t* gt_cat, const uint8_t* gt_counted, const uint8_t* gt_free,
                        const uint8_t* kind, const int64_t* partner, const uint8_t* missed, int32_t* fix_dt_match, uint8_t* fix_dt_ignore,
                        uint8_t* fix_gt_ignore, int32_t* cls_cat, int32_t* cls_match, uint8_t* cls_ignore, void* stream);

/* ---- Weighted boxes fusion (csrc/fusion_kernels.hip): two or more result sets, or several passes of one model, merged into one by
 * weighted boxes fusion (Solovyev, Wang, Gabruseva 2021).  The rule below is stated from the paper and from memory of its authors' package
 * `ensemble-boxes`, with three stated deviations; it was not run against that package.  The front end (object_detectors_amd/ensemble.py)
 * makes the candidates and the groups; the entry point clusters every group in one launch.
 * The rule (float64 throughout, no contraction, IEEE division).
 *   Inputs.  M >= 1 result sets, model m with weight w_m > 0; iou_thr in [0, 1) (default 0.55), skip_box_thr (default 0), conf_type avg or
 *     max.  W = w_0 + .. + w_{M-1} summed in that order, wmax = the largest weight.
 *   Candidates.  A detection (image, category, score s, box [x, y, w, h]) of model m becomes a candidate with s' = s * w_m and the corners
 *     x1 = x, y1 = y, x2 = x + w, y2 = y + h.  It is dropped, for the first reason that holds, when its image is unknown; s < skip_box_thr;
 *     s' is not finite or s' <= 0 (deviation 1: the package keeps a zero score and divides by it); x, y, w, h, x2 or y2 is not finite;
 *     w <= 0 or h <= 0.
 *   Groups and order.  A group is one (image, category) pair; its candidates stand in descending s', ties by model index, then by the order
 *     added: a stable sort over the model-major concatenation (deviation 2: the package's argsort is reversed and unstable).
 *   Clustering.  A group starts without clusters.  A cluster keeps its member count n, the sums S1..S4 and C, the maximum mx and its fused box
 *     F = (X1, Y1, X2, Y2).  For each candidate b in order and every cluster in creation order: iw = min(X2, b.x2) - max(X1, b.x1), iw <= 0
 *     gives the overlap 0, ih likewise in y, i = iw * ih, v = i / ((X2 - X1) * (Y2 - Y1) + (b.x2 - b.x1) * (b.y2 - b.y1) - i).  The cluster
 *     with the largest v is taken, the first made among equals.  v > iou_thr (strict): b joins it, n += 1, S_k = S_k + s' * coordinate_k (the
 *     product rounded first), C = C + s', mx = max(mx, s'), F_k = S_k / C.  Otherwise b founds a cluster: n = 1, S_k = s' * coordinate_k,
 *     C = mx = s' and F = the box itself, not S_k / C ((s' * x) / s' is not x for about one coordinate in ten).
 *   Scores, after the group's last candidate.  avg: score = ((C / n) * min(n, W)) / W with n as a double; max: score = mx / wmax
 *     (deviation 3: the package's box_and_model_avg, absent_model_aware_avg and allows_overflow are not provided).
 *   Result.  One detection per cluster: the group's image and category, the score, the box [X1, Y1, X2 - X1, Y2 - Y1] and members = n.
 * The entry point.  group_offsets [num_groups + 1] int64 ON THE DEVICE: group j owns the slots group_offsets[j]..group_offsets[j + 1] of
 *   boxes float64 [num_boxes, 4] (corners x1, y1, x2, y2) and scores float64 [num_boxes] (s'), both in fusion order; a slot no group owns is
 *   neither read nor written, and an empty group costs nothing.  num_groups and num_boxes are the caller's host copies: they size the arrays,
 *   a group whose offsets do not fit num_boxes is skipped, nothing is read or written past them; a group has no size cap.
 *   conf_type 0 = avg, 1 = max; weight_sum = W, weight_max = wmax.
 *   A cluster is identified with the slot of its founder.  Outputs, every array with num_boxes leading entries: leader int64 (per candidate:
 *   the founder slot of the cluster it ended in, its own slot for a founder) and founders int64 (row group_offsets[j] + c: the founder slot of
 *   group j's cluster c, creation order; the other rows of a group are not written); written AT FOUNDER SLOTS ONLY: sums float64 [*, 6]
 *   (S1..S4, C, mx), fused float64 [*, 4] (F as corners), out_scores float64 and members int32.  The caller finds the founders by
 *   leader[slot] == slot (after filling leader with -1 where slots may belong to no group) and compacts them; there is no count pass.
 * One wavefront per group, cluster c of a group always on lane c % 64; the fused boxes of a group's first mi355det_wbf_lds_clusters()
 * clusters are cached in LDS, the others are read back from `fused`.  Only the cluster that changed is re-divided.  No atomics, every element
 * has one writer, so the output is bit-identical from run to run.  No workspace.  MI355DET_EINVAL before any launch for a negative size, for
 * iou_thr outside [0, 1) or NaN, an unknown conf_type, weight_sum or weight_max not positive and finite, and for a missing operand with
 * num_boxes > 0; no launch when there are no groups or no boxes. */
int mi355det_wbf_lds_clusters(void);
int mi355det_wbf_fuse(const int64_t* group_offsets, int64_t num_groups, int64_t num_boxes, const double* boxes, const double* scores,
                      double iou_thr, int32_t conf_type, double weight_sum, double weight_max, int64_t* leader, int64_t* founders, double* sums,
                      double* fused, double* out_scores, int32_t* members, void* stream);

/* ---- Pooled precision-recall (csrc/pooled_kernels.hip): AP-pool of Dave et al., "Evaluating Large-Vocabulary Object Detectors: The Devil
 * is in the Details" (2021) - all categories' detections ranked in one list, one precision-recall curve - on the match arrays of the "COCO
 * evaluation" block above.  The paper's fork of lvis-api is not installed where this was written: the rules below are restated from memory
 * of the paper and of that fork, and the tests compare against a literal host form of this text.
 *   Pools.  A pool is a set of categories; its list is every detection slot of those categories that survives the evaluator's largest cut, in
 *     descending dt_score, stable over the slot index.  The caller builds the lists (a mask and a stable sort) and concatenates them:
 *     pool_order [num_order] int64, pool s owns pool_offsets[s]..pool_offsets[s + 1] (int64 [num_pools + 1] ON THE DEVICE;
 *     pool_offsets_host is the caller's HOST copy of the same table: it sizes the launches, the one host read of the caller).  An entry of
 *     pool_order outside 0..num_dt - 1 keeps its position and counts as ignored.  pool_npig [num_pools, num_areas] int64 on the device: the
 *     pool's ground truths with gt_ignore[a] == 0, summed by the caller.
 *   Per (pool s, area range a, threshold t), walking the list: tp counts the slots with dt_match != 0 and dt_ignore == 0, fp those with
 *     dt_match == 0 and dt_ignore == 0 (dt_match, dt_ignore [num_areas, num_thrs, num_dt] as the match entries write them); rc = tp / npig;
 *     pr = tp / (fp + tp + 2^-52), made non-increasing from the right; precision / scores [num_thrs, num_recs, num_pools, num_areas] = pr and
 *     dt_score at the first position with rc >= rec_thrs[r], 0 past the end; recall [num_thrs, num_pools, num_areas] = the last rc, 0 for an
 *     empty list; everything -1 where npig == 0.  These are coco_accumulate's expressions in float64 without contraction: a pool equals
 *     coco_accumulate on a single category that holds the pool's slots, bit for bit.
 *   How.  The list is cut into tiles of mi355det_pooled_tile() positions, one wavefront per tile and pass; the phases are separate launches
 *     and no kernel waits on another workgroup.  One gather pass packs each position's flags into a 64-bit tp mask and a 64-bit fp mask (bit
 *     a * num_thrs + t) and leaves the tile totals; their scan, the tiles' largest precision and its maximum over the later tiles are small
 *     tables between launches; the last pass lets every true positive write the thresholds it is the first to reach.  No atomics, one writer
 *     per output element, 64-bit positions: bit-identical from run to run.
 *   workspace: mi355det_pooled_accumulate_workspace(num_order, num_pools, num_thrs, num_areas) bytes on the device (0 for arguments the
 *     entry refuses), 16-byte aligned; its contents mean nothing to the caller.
 * MI355DET_EINVAL before any launch for a negative size; num_pools, num_thrs, num_areas or num_recs <= 0; num_thrs * num_areas > 64;
 * num_recs > 4096; a missing operand; host offsets that decrease, start below 0 or end past num_order; a workspace that is too small.  With
 * num_order == 0 the call writes the 0 / -1 cells and returns. */
int mi355det_pooled_tile(void);
size_t mi355det_pooled_accumulate_workspace(int64_t num_order, int32_t num_pools, int32_t num_thrs, int32_t num_areas);
int mi355det_pooled_accumulate(const int64_t* pool_order, int64_t num_order, const int64_t* pool_offsets, const int64_t* pool_offsets_host,
                               int32_t num_pools, const int64_t* pool_npig, int64_t num_dt, const double* dt_score, const int32_t* dt_match,
                               const uint8_t* dt_ignore, int32_t num_thrs, int32_t num_areas, const double* rec_thrs, int32_t num_recs,
                               double* precision, double* recall, double* scores, void* workspace, size_t workspace_bytes, void* stream);

/* layout / dtype converters at the module boundary */
int mi355det_nhwc_to_nchw_f32(const void* x, int x_is_bf16, int32_t x_ld, int32_t n, int32_t c, int32_t h,
                              int32_t w, float* out, void* stream);
int mi355det_nchw_f32_to_nhwc(const float* x, int32_t n, int32_t c, int32_t h, int32_t w, void* out,
                              int out_is_bf16, int32_t out_ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355DET_H */
