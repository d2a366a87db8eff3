"""Golden vectors of the run-length mask codec (tests/golden/rle.npz).

Runs in the build container only: it executes the reference's OWN mask_to_rle_pytorch / rle_to_mask / area_from_rle
(model/segment_anything_2/sam2/utils/amg.py) through _ref_import.functions on small masks made here, and records inputs
and outputs.  Nothing of the reference is copied; tests read the .npz only.

  python tests/golden/make_golden_rle.py
"""
import os
import sys
from typing import Any, Dict, List

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as ri  # noqa: E402
from make_golden_grounding import H, W, masks as grounding_masks  # noqa: E402


def masks():
    """the constructed set of the grounding fixture, plus the cases that are the codec's own: what happens at a column's end"""
    m = list(grounding_masks())

    def new():
        m.append(np.zeros((H, W), bool))
        return m[-1]

    a = new()                                          # (H-1, x) and (0, x+1): neighbours in column-major order, ONE run of 2
    a[H - 1, 20] = a[0, 21] = True
    a = new()                                          # (H-1, x) and (1, x+1): two runs
    a[H - 1, 20] = a[1, 21] = True
    yy, xx = np.mgrid[:H, :W]
    m.append((yy + xx) % 2 == 0)                       # checkerboard at even H: a column's last pixel equals the next one's first
    m.append((yy + xx) % 2 == 1)
    a = new()                                          # checkerboard at odd H (39 rows), the last row empty
    a[:H - 1] = ((yy + xx) % 2 == 0)[:H - 1]
    new()                                              # an empty mask between two non-empty ones
    new()[3:30, W - 1] = True                          # foreground in the last column only ...
    new()[:, W - 2:] = True                            # ... and the last two columns whole: the code ends on a foreground run
    new()[:, 0] = True                                 # the first column whole: a leading 0
    return np.stack(m)


# codes that no encoder here produces: zero counts inside (compressed COCO codes hold them), at the front and at the end
ZERO_CODES = [[0, 0, 5, 0, 0, 7, H * W - 12], [3, 0, 0, 0, 4, H * W - 7, 0], [0, H * W, 0, 0], [H * W, 0], [10, 5, 0, 5, H * W - 20],
              [0, 0, 0, H * W]]


def main():
    ns = {"torch": torch, "np": np, "Any": Any, "Dict": Dict, "List": List}
    mask_to_rle_pytorch, rle_to_mask, area_from_rle = ri.functions(
        "model/segment_anything_2/sam2/utils/amg.py", ["mask_to_rle_pytorch", "rle_to_mask", "area_from_rle"], ns)
    m = masks()
    rles = mask_to_rle_pytorch(torch.from_numpy(m))
    assert all(r["size"] == [H, W] for r in rles)
    for r, x in zip(rles, m):                                                      # the reference's own round trip
        assert np.array_equal(rle_to_mask(r), x) and area_from_rle(r) == x.sum()
    lens = [len(r["counts"]) for r in rles]
    out = {"masks": np.packbits(m, axis=-1), "shape": np.array(m.shape, np.int64),
           "counts": np.array([v for r in rles for v in r["counts"]], np.int32),
           "offsets": np.concatenate(([0], np.cumsum(lens))).astype(np.int64),
           "area": np.array([area_from_rle(r) for r in rles], np.int64)}
    zlens = [len(c) for c in ZERO_CODES]
    out["zero_counts"] = np.array([v for c in ZERO_CODES for v in c], np.int32)
    out["zero_offsets"] = np.concatenate(([0], np.cumsum(zlens))).astype(np.int64)
    out["zero_masks"] = np.packbits(np.stack([rle_to_mask({"size": [H, W], "counts": c}) for c in ZERO_CODES]), axis=-1)
    out["zero_area"] = np.array([area_from_rle({"size": [H, W], "counts": c}) for c in ZERO_CODES], np.int64)
    path = os.path.join(HERE, "rle.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, f"{os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
