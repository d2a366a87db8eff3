"""Mask post-processing and evaluation metrics on the device.

Same names, argument meaning and return values as the reference's helpers, but the masks stay in HBM: the pixel work
(connected components, boundary maps, dilation, intersections) runs in videoglamm_amd/csrc/vg_postproc.hip and only
a handful of integer counts per mask pair cross PCIe; the scalar arithmetic on those counts (divisions, the greedy
pairing of compute_miou, the F formula) is the reference's float64 host arithmetic.

  remove_small_blobs           R/eval_gcg_infer.py:20-29
  get_connected_components     R/model/segment_anything_2/sam2/utils/misc.py:47-63
  fill_holes_in_mask_scores    R/model/segment_anything_2/sam2/utils/misc.py:216-227
  compute_iou / compute_miou   R/eval_gcg_metrics.py:26-60
  db_eval_iou                  R/eval_referdavis_metrics.py:147-176   (void_pixels is not supported)
  db_eval_boundary / f_measure R/eval_referdavis_metrics.py:178-259
  masks_to_boxes               R/utils/grounding_utils/box_ops.py:118-142   (min_size: this build's extension)
  np_box_area / np_box_iou     R/utils/grounding_utils/box_ops.py:12-62     (the reference's numpy arithmetic, on the host)
  calc_tiou                    R/eval_grounding.py:55-72                    (_calc_tiou)
  video_grounding_metrics      R/eval_grounding.py:326-405                  (the per-video record of the VidSTG / HC-STVG driver)
  intersectionAndUnionGPU      R/utils/utils.py:78-90                       (K = 2; no write into `output`)
  validation_counts / validation_record / ValidationMeter
                               R/utils/trainer.py:413-465                   (the validator's gIoU / cIoU; the fused counts, N > 1
                               objects and the single-process meter are this build's forms)
  mask_to_rle_pytorch / rle_to_mask / area_from_rle / coco_encode_rle
                               R/model/segment_anything_2/sam2/utils/amg.py:109-155, 296-302   (coco_decode_rle, the compressed string
                               as input and device= are this build's extensions; the string codec is pycocotools' rule, in Python)
"""
import numpy as np
import torch

from . import ops


DEVICE = "cuda"     # where host inputs (numpy arrays / CPU tensors) are uploaded to


def _dev(x):
    """numpy / torch, host / device -> device tensor (bool stays bool)."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x if x.is_cuda else x.to(DEVICE)


def _mask(x):
    x = _dev(x)
    return x if x.dtype in (torch.bool, torch.uint8) else x != 0


def remove_small_blobs(binary_mask, min_size=0):
    """clear 4-connected blobs of fewer than min_size pixels; [..., H, W] (every leading index is its own image).
    Returns a device tensor of the input's dtype (uint8 for numpy bool input)."""
    m = _mask(binary_mask)
    if min_size <= 0:
        return m
    out = ops.remove_small_blobs(m, min_size)
    return out.view(torch.bool) if m.dtype == torch.bool else out


def get_connected_components(mask):
    """mask [N,1,H,W] (1 = foreground) -> (labels, counts) int32 [N,1,H,W], 8-connectivity."""
    return ops.connected_components(_mask(mask), 8)


def fill_holes_in_mask_scores(mask, max_area):
    assert max_area > 0, "max_area must be positive"
    return ops.fill_holes(_dev(mask).float(), max_area)


def iou_matrix(pred_masks, gt_masks):
    """[P, ...] x [G, ...] -> float64 [P, G] of |p & g| / |p | g| (nan where both are empty, like compute_iou)."""
    inter, uni = ops.mask_pair_counts(_mask(pred_masks), _mask(gt_masks))
    inter, uni = inter.cpu().numpy(), uni.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / uni


def compute_iou(mask1, mask2):
    return iou_matrix(_mask(mask1)[None], _mask(mask2)[None])[0, 0]


def compute_miou(pred_masks, gt_masks):
    """greedy one-to-one pairing by descending IoU, mean of the paired IoUs (0.0 when nothing pairs)."""
    pred_masks, gt_masks = list(pred_masks), list(gt_masks)
    if not pred_masks or not gt_masks:
        return 0.0
    iou = iou_matrix(torch.stack([_mask(p) for p in pred_masks]), torch.stack([_mask(g) for g in gt_masks]))
    paired = []
    while iou.size > 0 and np.max(iou) > 0:
        i, j = np.unravel_index(np.argmax(iou, axis=None), iou.shape)
        paired.append(iou[i, j])
        iou = np.delete(iou, i, axis=0)
        iou = np.delete(iou, j, axis=1)
    return np.mean(paired) if paired else 0.0


def db_eval_iou(annotation, segmentation, void_pixels=None):
    """per-frame Jaccard of [H,W] or [T,H,W] masks; 1 where the union is empty."""
    if void_pixels is not None:
        raise NotImplementedError("void_pixels are not used on this path (R/eval_referdavis_metrics.py passes None)")
    a, s = _mask(annotation), _mask(segmentation)
    assert a.shape == s.shape, f"Annotation({tuple(a.shape)}) and segmentation:{tuple(s.shape)} dimensions do not match."
    inter, uni = ops.mask_pair_counts(a.reshape(-1, *a.shape[-2:]), s.reshape(-1, *s.shape[-2:]), diagonal=True)   # all frames, one launch
    inter, uni = inter.cpu().numpy(), uni.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        j = inter / uni
    j[np.isclose(uni, 0)] = 1
    return j[0] if a.dim() == 2 else j


def _f_from_counts(n_fg, n_gt, fg_match, gt_match):
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1, 0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0, 1
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1, 1
    else:
        precision = fg_match / float(n_fg)
        recall = gt_match / float(n_gt)
    if precision + recall == 0:
        return 0
    return 2 * precision * recall / (precision + recall)


def db_eval_boundary(annotation, segmentation, void_pixels=None, bound_th=0.008):
    """boundary F-measure per frame of [H,W] or [T,H,W] masks."""
    if void_pixels is not None:
        raise NotImplementedError("void_pixels are not used on this path (R/eval_referdavis_metrics.py passes None)")
    a, s = _mask(annotation), _mask(segmentation)
    assert a.shape == s.shape
    if a.dim() not in (2, 3):
        raise ValueError(f"db_eval_boundary does not support tensors with {a.dim()} dimensions")
    H, W = a.shape[-2:]
    radius = int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((H, W))))
    counts = ops.boundary_counts(s, a, radius).cpu().numpy()
    f = np.array([_f_from_counts(*(int(v) for v in row)) for row in counts], dtype=np.float64)
    return f[0] if a.dim() == 2 else f


def f_measure(foreground_mask, gt_mask, void_pixels=None, bound_th=0.008):
    return db_eval_boundary(gt_mask, foreground_mask, void_pixels, bound_th)


# ---------------------------------------------------------------- grounding evaluation (VidSTG / HC-STVG): boxes, tIoU, vIoU
def boxes_xyxy(table):
    """int32 [..., 5] of ops.mask_boxes -> float32 [..., 4] as the reference's masks_to_boxes gives it: inclusive maxima,
    [1e8, 1e8, 0, 0] for an empty mask (its masked_fill value under min, and the max of an all-zero product)."""
    empty = table[..., 4:5] == 0
    fill = torch.tensor([1e8, 1e8, 0.0, 0.0], dtype=torch.float32, device=table.device)
    return torch.where(empty, fill, table[..., :4].to(torch.float32))


def masks_to_boxes(masks, min_size=0):
    """[N, H, W] masks -> float32 device tensor [N, 4] = (x_min, y_min, x_max, y_max), zeros((0, 4)) for no pixels at all.
    The reduction runs where the masks are (ops.mask_boxes): 20 bytes per mask leave the device, and only when the caller
    asks for host values.  min_size > 0 gives the boxes of remove_small_blobs(mask, min_size) in the same chain."""
    m = _mask(masks)
    if m.numel() == 0:
        return torch.zeros((0, 4), dtype=torch.float32, device=m.device)
    return boxes_xyxy(ops.mask_boxes(m, min_size))


def np_box_area(boxes):
    assert boxes.ndim == 2 and boxes.shape[-1] == 4
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def _box_inter_union(boxes1, boxes2):
    area1, area2 = np_box_area(boxes1), np_box_area(boxes2)
    lt = np.maximum(boxes1[:, None, :2], boxes2[:, :2])
    rb = np.minimum(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clip(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter, area1[:, None] + area2 - inter


def np_box_iou(boxes1, boxes2):
    """[N, 4] x [M, 4] (x1, y1, x2, y2) -> [N, M]; numpy's own dtype promotion and division (a degenerate pair divides by 0)."""
    inter, union = _box_inter_union(boxes1, boxes2)
    return inter / union


def calc_tiou(gt_sted, pred_sted, frame_ids):
    """(tiou, frames of the union span, set of frames of the intersection span); spans are [start, end)."""
    max_start, min_end = max(gt_sted[0], pred_sted[0]), min(gt_sted[1], pred_sted[1])
    min_start, max_end = min(gt_sted[0], pred_sted[0]), max(gt_sted[1], pred_sted[1])
    if min_end <= max_start:
        tiou = 0
    else:
        intersection = min_end - max_start
        tiou = intersection / ((gt_sted[1] - gt_sted[0]) + (pred_sted[1] - pred_sted[0]) - intersection)
    union_predgt = [f for f in frame_ids if min_start <= f < max_end]
    inter_predgt = set(f for f in frame_ids if max_start <= f < min_end)
    return tiou, union_predgt, inter_predgt


def _box14(b):
    if torch.is_tensor(b):
        b = b.detach().cpu().numpy()
    return np.asarray(b).reshape(1, 4)


def video_grounding_metrics(pred_boxes, gt_boxes, gt_sted, frame_ids, pred_sted=None, iou_thresholds=(0.3, 0.5)):
    """The per-video record of R/eval_grounding.py:326-405.  pred_boxes / gt_boxes: {frame: box [4] or [1, 4]}; gt_sted: the
    annotated moment, both ends INCLUSIVE here (the driver iterates range(gt_sted[0], gt_sted[1] + 1)); pred_sted: the predicted
    span when the model localises in time (the driver's tmp_loc), which adds tiou / viou / viou@thr.
    ONE box per frame: the driver overwrites predictions[t] in its loop over the objects of a frame (:281-287), so it scores the
    LAST object's box; which object to score is the caller's choice here.
    A frame of the annotated moment without a prediction raises RuntimeError, as the driver does."""
    rec = {"img_metrics": {}}
    if pred_sted is not None:
        tiou, union_predgt, inter_predgt = calc_tiou(gt_sted, pred_sted, frame_ids)
        rec.update(gt_sted=gt_sted, pred_sted=pred_sted, tiou=tiou)
    inter_frames = list(range(gt_sted[0], gt_sted[1] + 1))
    viou = gt_viou = 0
    for f in inter_frames:
        if f not in pred_boxes:
            raise RuntimeError(f"No prediction for frame {f}")
        pb, gb = _box14(pred_boxes[f]), _box14(gt_boxes[f])
        iou = np_box_iou(pb, gb)[0][0]
        rec["img_metrics"][f] = {"iou": iou, "pred_box": pb[0], "gt_box": gb[0]}
        if pred_sted is not None and f in inter_predgt:
            viou += iou
        gt_viou += iou
    if pred_sted is not None:
        viou = viou / max(len(union_predgt), 1)
        rec["viou"] = viou
        rec.update({f"viou@{t}": int(viou > t) for t in iou_thresholds})
    gt_viou = gt_viou / max(len(inter_frames), 1)
    rec["gt_viou"] = gt_viou
    rec.update({f"gt_viou@{t}": int(gt_viou > t) for t in iou_thresholds})
    return rec


# ---------------------------------------------------------------- validation (gIoU / cIoU): class counts from logits, ignore label included
def _labels_u8(target):
    """a ground truth as the validator holds it (bool, integer, or float labels it would .int()) -> device tensor that
    ops.logit_class_counts takes: bool / uint8 as they are, anything else as integers (range-checked there)"""
    t = _dev(target)
    if t.dtype in (torch.bool, torch.uint8):
        return t
    return t.long() if t.dtype.is_floating_point else t


def intersectionAndUnionGPU(output, target, K, ignore_index=255):
    """Label tensors (0 / 1 in output, 0 / 1 / ignore_index in target) of 1 to 3 dimensions -> (area_intersection, area_union,
    area_target), float32 device tensors [K], the values the reference returns for float input.  K must be 2.  Runs on
    vg_logit_class_counts: the labels go in as float32 logits, output > 0 being the label for labels 0 / 1 (any other value in
    output is outside this function's domain).  The reference also WRITES ignore_index into `output` where the target has it
    (its callers pass a clone); that side effect is not reproduced: `output` is left as it is."""
    if K != 2:
        raise NotImplementedError(f"intersectionAndUnionGPU: K = {K}; the validator's two classes (K = 2) are what the kernel counts")
    assert len(output.shape) in [1, 2, 3]
    assert tuple(output.shape) == tuple(target.shape)
    out = _dev(output)
    if out.numel() == 0:
        z = torch.zeros(2, dtype=torch.float32, device=out.device)
        return z, z.clone(), z.clone()
    c = ops.logit_class_counts(out.reshape(1, -1).to(torch.float32), _labels_u8(target).reshape(1, -1), ignore_index)
    inter, area_out, area_tgt = c[0:2], c[2:4], c[4:6]
    return inter.to(torch.float32), (area_out + area_tgt - inter).to(torch.float32), area_tgt.to(torch.float32)


def validation_counts(pred_logits, gt_masks, ignore_index=255):
    """The fused path of the validator's metric: mask logits [N, T, H, W] or [T, H, W] (float32 / bf16, on the device) and the
    ground truth of the same shape (0 / 1 / ignore_index) -> int64 [.., T, 6] = (inter0, inter1, out0, out1, tgt0, tgt1) per
    frame, all frames and objects in ONE launch: no thresholded copy, no clone, no histograms."""
    if pred_logits.dim() not in (3, 4) or tuple(pred_logits.shape) != tuple(gt_masks.shape):
        raise ValueError(f"validation_counts: logits {tuple(pred_logits.shape)} and ground truth {tuple(gt_masks.shape)} must be equal "
                         "[N, T, H, W] or [T, H, W] shapes")
    return ops.logit_class_counts(pred_logits, _labels_u8(gt_masks), ignore_index)


def record_from_counts(table):
    """The validator's per-sample arithmetic (R/utils/trainer.py:442-453) on a host table [T, 6] or [N, T, 6] of
    validation_counts: (intersection float32 [2], union float32 [2], acc_iou float32 [2], n).  In the reference's float32
    and in its order: per frame intersection += inter_i, union += union_i, acc_iou += inter_i / (union_i + 1e-5), + 1.0
    where union_i == 0 (no-object target); acc_iou / n at the end.  The N * T (object, frame) rows of an [N, T, 6] table
    enter alike, object-major, and n = N * T; for N = 1 that is the reference's value."""
    c = torch.as_tensor(np.asarray(table)).reshape(-1, 6)
    n = c.shape[0]
    inter = c[:, 0:2].to(torch.float32)
    uni = (c[:, 2:4] + c[:, 4:6] - c[:, 0:2]).to(torch.float32)
    intersection, union, acc_iou = torch.zeros(2), torch.zeros(2), torch.zeros(2)
    for inter_i, union_i in zip(inter, uni):
        intersection += inter_i
        union += union_i
        acc_iou += inter_i / (union_i + 1e-5)
        acc_iou[union_i == 0] += 1.0
    return intersection.numpy(), union.numpy(), acc_iou.numpy() / n, n


def validation_record(output_dict, ignore_index=255):
    """R/utils/trainer.py:413-456 for one sample of model_forward(inference=True): pred_masks[0] (T tensors [N, H, W] of
    logits) stacked to [N, T, H, W] on the device, gt_masks[0] ([N, T, H, W]; 0 / 1 / ignore_index), one validation_counts
    call, one download of N * T * 48 bytes, record_from_counts.  Returns (intersection, union, acc_iou, n).
    The reference asserts one object; N > 1 is this build's extension (record_from_counts).  A prediction without objects
    (the [0, H, W] tensors model_forward returns when no [SEG] was emitted) counts as all-background logits for every object
    of the ground truth: the reference would fail on it, and a missed object is what the metric should charge."""
    gt = _labels_u8(output_dict["gt_masks"][0])
    pred = torch.stack(list(output_dict["pred_masks"][0]), dim=0).permute(1, 0, 2, 3)
    if pred.shape[0] == 0:
        pred = torch.zeros(gt.shape, dtype=torch.float32, device=gt.device)
    return record_from_counts(validation_counts(pred, gt, ignore_index).cpu().numpy())


class ValidationMeter:
    """The three meters of the validator (R/utils/trainer.py:454-465 over R/utils/utils.py AverageMeter) in one object, on the
    host, one process (no all_reduce): update(record) takes what validation_record returns, result() gives (giou, ciou) =
    (acc_iou_sum / count)[1], (intersection_sum / (union_sum + 1e-10))[1].  The sums keep the dtype numpy gives the
    reference's own expressions (val * n added to a Python 0), which is the records' float32."""

    def __init__(self):
        self.intersection_sum = self.union_sum = self.acc_iou_sum = 0
        self.count = 0

    def update(self, record):
        intersection, union, acc_iou, n = record
        self.intersection_sum += intersection * 1
        self.union_sum += union * 1
        self.acc_iou_sum += acc_iou * n
        self.count += n

    def result(self):
        if self.count == 0:
            raise ValueError("ValidationMeter.result() before any update()")
        iou_class = self.intersection_sum / (self.union_sum + 1e-10)
        acc_iou_avg = self.acc_iou_sum / self.count
        return float(acc_iou_avg[1]), float(iou_class[1])


# ---------------------------------------------------------------- run-length codes (COCO RLE): the form masks are stored and exchanged in
def _split_rle(counts, offsets, size):
    """host counts / offsets of ops.mask_rle -> one {"size", "counts"} per mask"""
    c, o = counts.tolist(), offsets.tolist()
    return [{"size": list(size), "counts": c[a:b]} for a, b in zip(o[:-1], o[1:])]


def mask_to_rle_pytorch(masks):
    """[N, H, W] masks -> [{"size": [h, w], "counts": [int, ...]}, ...], COCO's uncompressed RLE: runs of the column-major pixel order,
    background first (a leading 0 when pixel 0 is foreground).  Encoded where the masks are (ops.mask_rle); the counts cross PCIe."""
    m = _mask(masks)
    assert m.dim() == 3, "mask_to_rle_pytorch takes [N, H, W]"
    if m.shape[0] == 0:
        return []
    counts, offsets = ops.mask_rle(m)
    return _split_rle(counts.cpu(), offsets.cpu(), m.shape[-2:])


def coco_encode_rle(rle):
    """uncompressed code -> {"size", "counts": str}: pycocotools' rleToString.  Each count (minus the count two places back from the fourth
    on) goes out in 5-bit groups, low group first; bit 5 of a character says that another group follows, and bit 4 of the last group is
    the sign.  Pinned to this statement and to the vector in the tests: pycocotools itself is not a dependency."""
    cnts = rle["counts"]
    if isinstance(cnts, (str, bytes)):
        return {"size": list(rle["size"]), "counts": cnts if isinstance(cnts, str) else cnts.decode("ascii")}
    s = []
    for i, x in enumerate(cnts):
        x = int(x)
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if c & 0x10 else (x != 0)
            if more:
                c |= 0x20
            s.append(chr(c + 48))
    return {"size": list(rle["size"]), "counts": "".join(s)}


def coco_decode_rle(rle):
    """{"size", "counts": str or bytes} -> uncompressed code: pycocotools' rleFrString.  A code that already holds a count list is copied."""
    s = rle["counts"]
    if not isinstance(s, (str, bytes)):
        return {"size": list(rle["size"]), "counts": [int(v) for v in s]}
    if isinstance(s, str):
        s = s.encode("ascii")
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError("coco_decode_rle: the string ends inside a count")
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return {"size": list(rle["size"]), "counts": cnts}


def area_from_rle(rle):
    return sum(coco_decode_rle(rle)["counts"][1::2])


def rle_to_mask(rle, device=None):
    """One code -> bool ndarray [h, w] (the reference's value); a list of codes -> a list of them.  Codes hold count lists or compressed
    strings.  device: keep the result there and return bool device tensor(s), so that a stored ground truth reaches the metrics of this
    module as its counts (kilobytes) and not as a dense upload.  Decoded on the device (ops.rle_to_mask), all codes of one size in one call;
    a code with a negative count, or whose counts do not sum to h * w, raises ValueError."""
    single = isinstance(rle, dict)
    codes = [coco_decode_rle(r) for r in ([rle] if single else rle)]
    dev = torch.device(DEVICE if device is None else device)
    out = [None] * len(codes)
    by_size = {}
    for i, r in enumerate(codes):
        by_size.setdefault(tuple(int(v) for v in r["size"]), []).append(i)
    for (h, w), ids in by_size.items():
        lens = [len(codes[i]["counts"]) for i in ids]
        flat = [v for i in ids for v in codes[i]["counts"]]
        if any(not -2 ** 31 <= v < 2 ** 31 for v in flat):
            raise ValueError("rle_to_mask: a count does not fit int32")
        counts = torch.tensor(flat, dtype=torch.int32).to(dev)
        offsets = torch.tensor(np.concatenate(([0], np.cumsum(lens, dtype=np.int64))), dtype=torch.int64).to(dev)
        masks, status = ops.rle_to_mask(counts, offsets, h, w)
        bad = status.cpu().nonzero().flatten().tolist()
        if bad:
            raise ValueError(f"rle_to_mask: the counts of code {ids[bad[0]]} are negative or do not sum to {h} * {w}")
        masks = masks.view(torch.bool) if device is not None else masks.cpu().numpy().view(bool)
        for k, i in enumerate(ids):
            out[i] = masks[k]
    return out[0] if single else out
