"""The grounding evaluation (VidSTG / HC-STVG) without a GPU: the host helpers of
videoglamm_amd/postproc.py against the reference's own outputs (tests/golden/grounding.npz, exact), the per-video record on
hand-computed clips, and masks_to_boxes / the façade's return_boxes with ops.mask_boxes replaced by its numpy statement
(tests/_boxes_ref.py)."""
import re

import numpy as np
import pytest
import torch

import _boxes_ref as BR
import _golden as G

torch.set_grad_enabled(False)


def gold():
    return {k: v.numpy() for k, v in G.fixture("grounding.npz").items()}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_statement_matches_reference_boxes():
    g = gold()
    assert same(BR.xyxy_np(g["masks"]), g["boxes"])
    assert (g["boxes"][0] == [1e8, 1e8, 0, 0]).all() and g["masks"][0].sum() == 0          # the empty-mask rule


def test_box_area_and_iou_match_reference():
    from videoglamm_amd import postproc as PP
    g = gold()
    b1, b2 = g["boxes1"], g["boxes2"]
    assert b1.dtype == np.float32 and b2.dtype == np.float64
    assert same(PP.np_box_area(b1), g["area1"]) and same(PP.np_box_area(b2), g["area2"])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert same(PP.np_box_iou(b1, b2), g["iou"]) and g["iou"].dtype == np.float64       # float32 x float64 -> float64
        assert same(PP.np_box_iou(b1, b2.astype(np.float32)), g["iou32"]) and g["iou32"].dtype == np.float32
    with pytest.raises(AssertionError):
        PP.np_box_area(b1[0])
    assert PP.np_box_iou(np.array([[0, 0, 2, 2]], np.float32), np.array([[1, 1, 3, 3]], np.float64))[0, 0] == 1 / 7


def test_tiou_matches_reference():
    from videoglamm_amd import postproc as PP
    g = gold()
    frame_ids = list(range(g["tiou_union"].shape[1]))
    for k, (gt, pred) in enumerate(g["tiou_sted"]):
        tiou, union, inter = PP.calc_tiou(tuple(int(v) for v in gt), tuple(int(v) for v in pred), frame_ids)
        assert np.float64(tiou) == g["tiou"][k]
        assert isinstance(union, list) and isinstance(inter, set)
        assert union == [f for f in frame_ids if g["tiou_union"][k, f]] and len(union) == g["tiou_union_len"][k]
        assert inter == {f for f in frame_ids if g["tiou_inter"][k, f]}
    assert PP.calc_tiou((0, 5), (5, 9), frame_ids)[0] == 0                                  # touching spans do not intersect


# ------------------------------------------------------------------------------------------------ the per-video record
GT = np.array([0, 0, 10, 10], np.float64)


def _pred(iou_num):
    """a box inside GT (area 100) with IoU iou_num / 100"""
    return np.array([[0, 0, 10, iou_num / 10]], np.float32)


def test_video_record_without_pred_sted():
    from videoglamm_amd import postproc as PP
    frames = list(range(6))
    pred = {f: _pred(v) for f, v in zip(frames, (50, 20, 40, 80, 100, 10))}
    gt = {f: GT for f in frames}
    rec = PP.video_grounding_metrics(pred, gt, (1, 3), frames)
    assert sorted(rec["img_metrics"]) == [1, 2, 3]
    assert [rec["img_metrics"][f]["iou"] for f in (1, 2, 3)] == [0.2, 0.4, 0.8]
    assert rec["img_metrics"][2]["iou"].dtype == np.float64                                  # float32 prediction, float64 ground truth
    assert same(rec["img_metrics"][1]["pred_box"], _pred(20)[0]) and same(rec["img_metrics"][1]["gt_box"], GT)
    assert rec["gt_viou"] == (0.2 + 0.4 + 0.8) / 3 and rec["gt_viou@0.3"] == 1 and rec["gt_viou@0.5"] == 0
    assert not any(k in rec for k in ("tiou", "viou", "viou@0.3", "pred_sted"))
    rec = PP.video_grounding_metrics(pred, gt, (4, 4), frames, iou_thresholds=(0.9, 1.0))
    assert rec["gt_viou"] == 1.0 and rec["gt_viou@0.9"] == 1 and rec["gt_viou@1.0"] == 0     # strict


def test_video_record_with_pred_sted():
    from videoglamm_amd import postproc as PP
    frames = list(range(8))
    pred = {f: _pred(v) for f, v in zip(frames, (10, 30, 50, 70, 90, 20, 40, 60))}
    gt = {f: GT.reshape(1, 4) for f in frames}
    # annotated moment 2..5 (inclusive); predicted span [4, 7): intersection span [4, 5) = {4}, union span [2, 7) = 5 frames;
    # tiou = 1 / (3 + 3 - 1) = 0.2
    rec = PP.video_grounding_metrics(pred, gt, (2, 5), frames, pred_sted=(4, 7))
    assert rec["tiou"] == 0.2 and rec["gt_sted"] == (2, 5) and rec["pred_sted"] == (4, 7)
    assert rec["viou"] == 0.9 / 5 and rec["viou@0.3"] == 0 and rec["viou@0.5"] == 0
    assert rec["gt_viou"] == (0.5 + 0.7 + 0.9 + 0.2) / 4 and rec["gt_viou@0.3"] == 1 and rec["gt_viou@0.5"] == 1
    # disjoint spans: no frame counts towards viou
    rec = PP.video_grounding_metrics(pred, gt, (2, 3), frames, pred_sted=(5, 7))
    assert rec["tiou"] == 0 and rec["viou"] == 0 and rec["viou@0.3"] == 0


def test_video_record_threshold_is_strict_and_missing_frame_raises():
    from videoglamm_amd import postproc as PP
    frames = [0, 1, 2]
    pred = {f: _pred(30) for f in frames}                 # 3 / 10 in float64 IS the literal 0.3
    gt = {f: GT for f in frames}
    rec = PP.video_grounding_metrics(pred, gt, (1, 2), frames, pred_sted=(1, 2))             # spans [1, 2): one frame each way
    assert rec["gt_viou"] == 0.3 and rec["gt_viou@0.3"] == 0                                 # (0.3 + 0.3) / 2, hit exactly: does not count
    assert rec["tiou"] == 1 and rec["viou"] == 0.3 and rec["viou@0.3"] == 0
    del pred[1]
    with pytest.raises(RuntimeError, match=re.escape("No prediction for frame 1")):
        PP.video_grounding_metrics(pred, gt, (0, 2), frames)
    rec = PP.video_grounding_metrics({}, gt, (2, 1), frames)                                 # an empty moment: max(len, 1)
    assert rec["gt_viou"] == 0 and rec["img_metrics"] == {}


# ------------------------------------------------------------------------------------------------ masks_to_boxes on the statement
@pytest.fixture()
def host_boxes(cpu_ops, monkeypatch):
    from videoglamm_amd import _lib, ops
    from videoglamm_amd import postproc as PP
    calls = []

    def mask_boxes(masks, min_size=0, return_mask=False):
        calls.append((tuple(masks.shape), min_size, return_mask))
        return BR.mask_boxes(masks, min_size, return_mask)

    monkeypatch.setattr(ops, "mask_boxes", mask_boxes, raising=True)
    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(PP, "DEVICE", "cpu")
    return calls


def test_masks_to_boxes_matches_reference(host_boxes, monkeypatch):
    from videoglamm_amd import postproc as PP
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))    # CPU tensors stand in for device tensors
    g = gold()
    for m in (g["masks"], g["masks"].astype(bool), torch.from_numpy(g["masks"]), torch.from_numpy(g["masks"]).bool(),
              g["masks"].astype(np.float32) * 3):
        out = PP.masks_to_boxes(m)
        assert torch.is_tensor(out) and same(out.numpy(), g["boxes"])
    out = PP.masks_to_boxes(np.zeros((0, 4, 5), bool))
    assert out.dtype == torch.float32 and tuple(out.shape) == (0, 4)
    m = g["masks"]
    assert same(PP.masks_to_boxes(m, min_size=20).numpy(), BR.xyxy_np(m, 20))
    assert not same(BR.xyxy_np(m, 20), g["boxes"])                                # the filter changes some of them
    assert host_boxes[-1] == (m.shape, 20, False)


# ------------------------------------------------------------------------------------------------ the façade
def _build(**over):
    from test_oracle_e2e import e2e_setup
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    fx, sd, cfg, inp = e2e_setup()
    kw = {k: over.pop(k) for k in ("min_blob_size",) if k in over}
    m = VideoGLaMMForCausalLM(sd, dict(cfg, **over), torch_dtype=torch.float32, device=torch.device("cpu"), **kw)
    args = ([inp["images"]], [inp["context_images"]], [inp["images_for_sam"]], inp["input_ids"][None], [(1024, 1024)], [inp["original_size"]])
    return m, args, inp


def check_boxes(segs, boxes):
    """the twin has the masks' keys, and every value is the statement's on the returned mask"""
    assert len(segs) == len(boxes) == 1
    seg, box = segs[0], boxes[0]
    assert len(seg) > 0 and list(seg) == list(box)
    for t in seg:
        assert list(seg[t]) == list(box[t])
        for k in seg[t]:
            b = box[t][k]
            assert isinstance(b, np.ndarray) and b.dtype == np.float32 and b.shape == (4,)
            assert np.array_equal(b, BR.xyxy_np(seg[t][k])), (t, k)


@pytest.mark.parametrize("video,blob", [(False, 0), (True, 20)])
def test_facade_return_boxes(host_boxes, video, blob):
    m, args, inp = _build(min_blob_size=blob)
    kw = dict(max_new_tokens=inp["max_new_tokens"], use_sam2_video_branch=video)
    ids, segs, boxes = m.inference(*args, return_boxes=True, **kw)
    calls = list(host_boxes)
    ref = m.inference(*args, return_boxes=False, **kw)                            # after the True call: the keyword does not stick
    assert isinstance(ref, tuple) and len(ref) == 2 and host_boxes == calls       # the old tuple, and no box reduction
    assert ids.equal(ref[0])
    seg, rseg = segs[0], ref[1][0]
    assert all(np.array_equal(seg[t][k], rseg[t][k]) for t in rseg for k in rseg[t]) and list(seg) == list(rseg)
    check_boxes(segs, boxes)
    T, N = len(seg), len(seg[0])
    assert calls == [((T, N) + tuple(inp["original_size"]), blob, blob > 0)]      # ONE call over all T x N masks


def test_facade_no_seg_and_refusal(host_boxes):
    m, args, inp = _build(seg_token_idx=10 ** 6)
    ids, segs, boxes = m.inference(*args, max_new_tokens=3, use_sam2_video_branch=True, return_boxes=True)
    assert segs == [{}] and boxes == [{}] and host_boxes == []
    m.comm = object()                                                             # a multi-GPU model
    with pytest.raises(NotImplementedError, match="return_boxes"):
        m.inference(*args, max_new_tokens=3, return_boxes=True)
    with pytest.raises(NotImplementedError, match="return_boxes"):
        m.inference_framewise(*args, max_new_tokens=3, return_boxes=True)


# ------------------------------------------------------------------------------------------------ ABI
def test_new_entry_points_are_declared_and_bound():
    import inspect
    import os
    from videoglamm_amd import _lib
    with open(os.path.join(os.path.dirname(G.HERE), "include", "vg_kernels.h")) as f:
        header = f.read()
    bound = inspect.getsource(_lib._sig)
    for name in ("vg_mask_boxes", "vg_blob_boxes"):
        assert re.search(rf"\bint {name}\(", header) and f'"{name}"' in bound
