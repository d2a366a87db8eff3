"""Golden vectors of the grounding evaluation's host helpers (tests/golden/grounding.npz).

Runs in the build container only: it executes the reference's OWN masks_to_boxes / np_box_area / _box_inter_union /
np_box_iou (utils/grounding_utils/box_ops.py) and _calc_tiou (eval_grounding.py) through _ref_import.functions on small
inputs made here, and records inputs and outputs.  Nothing of the reference is copied; tests read the .npz only.

  python tests/golden/make_golden_grounding.py
"""
import os
import sys
from typing import Tuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as ri  # noqa: E402

H, W = 40, 50


def masks():
    rng = np.random.default_rng(20)
    m = []

    def new():
        m.append(np.zeros((H, W), bool))
        return m[-1]

    new()                                              # empty
    new()[:] = True                                    # full
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (17, 23)):
        new()[y, x] = True                             # single pixels: the four corners and an inner one
    new()[7, :] = True                                 # one row
    new()[:, 31] = True                                # one column
    new()[0, 3:9] = True                               # a run on the first row
    new()[5:9, W - 1] = True                           # a run on the last column
    a = new()                                          # two far blobs
    a[2:5, 3:8] = True
    a[30:38, 40:49] = True
    a = new()                                          # pixel (y, W-1) and pixel (y+1, 0): the row end
    a[11, W - 1] = a[12, 0] = True
    a = new()
    a[10:30, 10:40] = True                             # a rectangle with a hole
    a[15:20, 20:30] = False
    for d in (0.02, 0.02, 0.02, 0.5, 0.5, 0.5):
        m.append(rng.random((H, W)) < d)
    for hh, ww in ((1, 1), (1, 17), (5, 7), (3, 16)):  # small images embedded top-left, rest empty
        new()[:hh, :ww] = rng.random((hh, ww)) < 0.5
    return np.stack(m)


def box_pairs():
    """rows of boxes1 against rows of boxes2 (the reference computes the full [N, M] matrix)"""
    b1 = np.array([[0, 0, 10, 10], [2, 2, 4, 4], [0, 0, 5, 5], [3, 4, 9, 12], [7, 7, 7, 7], [1e8, 1e8, 0, 0],
                   [10.5, 3.25, 20.75, 8.5], [0, 0, 1, 1], [5, 5, 15, 15], [0, 0, 49, 39], [20, 0, 30, 39], [4, 4, 6, 6]], np.float32)
    b2 = np.array([[20, 20, 30, 30], [0, 0, 10, 10], [5, 0, 9, 5], [3, 4, 9, 12], [0, 0, 10, 10], [0, 0, 10, 10],
                   [12, 4, 18, 6], [1, 1, 2, 2], [10, 10, 20, 20], [0, 0, 49, 39], [25, 10, 45, 20], [7, 7, 7, 7]], np.float64)
    return b1, b2


TIOU = [((2, 8), (4, 10)), ((0, 5), (5, 9)), ((0, 5), (7, 9)), ((3, 9), (3, 9)), ((1, 12), (4, 6)), ((4, 6), (1, 12)),
        ((0, 1), (0, 1)), ((5, 5), (2, 9)), ((0, 15), (14, 15)), ((6, 9), (0, 7))]
FRAMES = 16


def main():
    ns = {"torch": torch, "np": np, "Tuple": Tuple}
    masks_to_boxes, np_box_area, _, np_box_iou = ri.functions(
        "utils/grounding_utils/box_ops.py", ["masks_to_boxes", "np_box_area", "_box_inter_union", "np_box_iou"], ns)
    (calc_tiou,) = ri.functions("eval_grounding.py", ["_calc_tiou"], ns)
    m = masks()
    out = {"masks": m.astype(np.uint8)}
    boxes = masks_to_boxes(torch.from_numpy(m))
    assert boxes.dtype == torch.float32 and torch.equal(boxes, masks_to_boxes(torch.from_numpy(m.astype(np.uint8))))    # bool == uint8
    assert tuple(masks_to_boxes(torch.zeros((0, H, W), dtype=torch.bool)).shape) == (0, 4)
    out["boxes"] = boxes.numpy()
    b1, b2 = box_pairs()
    out.update(boxes1=b1, boxes2=b2, area1=np_box_area(b1), area2=np_box_area(b2))
    with np.errstate(invalid="ignore", divide="ignore"):
        out["iou"] = np_box_iou(b1, b2)                 # float32 x float64 -> float64 [12, 12]
        out["iou32"] = np_box_iou(b1, b2.astype(np.float32))
    frame_ids = list(range(FRAMES))
    res = [calc_tiou(g, p, frame_ids) for g, p in TIOU]
    out["tiou_sted"] = np.array(TIOU, np.int64)                                    # [K, 2 (gt, pred), 2]
    out["tiou"] = np.array([r[0] for r in res], np.float64)
    out["tiou_union"] = np.array([[f in r[1] for f in frame_ids] for r in res])    # membership rows (the lists are ascending frame ids)
    out["tiou_inter"] = np.array([[f in r[2] for f in frame_ids] for r in res])
    out["tiou_union_len"] = np.array([len(r[1]) for r in res], np.int64)
    path = os.path.join(HERE, "grounding.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, f"{os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
