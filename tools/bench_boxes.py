"""Boxes from masks on the MI355X (vg_mask_boxes / vg_blob_boxes) against their yardsticks.
usage: python tools/bench_boxes.py [out.jsonl]      (default: profiles/bench_boxes.jsonl, appended)

  A  ops.mask_boxes(m)                                   the one-pass reduction
  B  ops.mask_boxes(m, 20)  vs  ops.mask_boxes(ops.remove_small_blobs(m, 20))      fused finalize vs the two calls
  C  the torch formula of masks_to_boxes on the same device tensors: two meshgrids, products, masked_fill, min / max

Every case is captured into a graph once and replayed; a sample is the device-event time of REPLAYS replays divided by REPLAYS,
a figure is the median of 20 samples, and the cases alternate inside each of ROUNDS rounds, so that drift hits them alike.  The
spread of a case is max - min of its rounds' medians (DESIGN 8c's rule: a difference is real beyond three times the larger spread)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videoglamm_amd import ops      # noqa: E402

SAMPLES, REPLAYS, ROUNDS = 20, 10, 3


def blobs(shape, seed, density=0.5, smooth=4):
    """seeded blobby masks (box-filtered noise above a quantile) with specks for the blob filter to remove"""
    rng = np.random.RandomState(seed)
    x = rng.rand(*shape).astype(np.float32)
    speck = rng.rand(*shape) < 0.001
    for ax in (-2, -1):
        for _ in range(smooth):
            x = (np.roll(x, 1, ax) + x + np.roll(x, -1, ax)) / 3
    return (x > np.quantile(x, 1 - density)) | speck


def torch_formula(masks):
    """the work masks_to_boxes does in the reference's utilities (R/utils/grounding_utils/box_ops.py:118-142), as plain torch on the device:
    per axis a full-size fp32 coordinate grid, its product with the masks, the row maximum of the product, and the row minimum of the
    product with the background filled with 1e8 — six [N, H, W] fp32 temporaries and four reductions over them"""
    H, W = masks.shape[-2:]
    grid_y, grid_x = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=masks.device),
                                    torch.arange(W, dtype=torch.float32, device=masks.device), indexing="ij")
    background = ~masks

    def extent(grid):
        coords = masks * grid[None]
        return coords.masked_fill(background, 1e8).flatten(1).min(-1).values, coords.flatten(1).max(-1).values

    (x_lo, x_hi), (y_lo, y_hi) = extent(grid_x), extent(grid_y)
    return torch.stack([x_lo, y_lo, x_hi, y_hi], 1)


def captured(fn):
    fn()                                    # warm: code objects, the allocator
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        keep = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, keep


def sample(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPLAYS * 1e3      # us


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_boxes.jsonl")
    dev = torch.device("cuda:0")
    lines = []
    for N in (32, 8):
        m = torch.from_numpy(blobs((N, 1024, 1024), N)).to(dev)
        from videoglamm_amd.postproc import boxes_xyxy
        assert torch.equal(boxes_xyxy(ops.mask_boxes(m)), torch_formula(m)), "the two sides of case C disagree"
        assert torch.equal(ops.mask_boxes(m, 20), ops.mask_boxes(ops.remove_small_blobs(m, 20))), "the two sides of case B disagree"
        cases = {"A mask_boxes": lambda: ops.mask_boxes(m),
                 "B mask_boxes(min_size=20)": lambda: ops.mask_boxes(m, 20),
                 "B remove_small_blobs(20) + mask_boxes": lambda: ops.mask_boxes(ops.remove_small_blobs(m, 20)),
                 "B remove_small_blobs(20) alone": lambda: ops.remove_small_blobs(m, 20),
                 "C torch formula": lambda: torch_formula(m)}
        graphs = {k: captured(fn) for k, fn in cases.items()}
        medians = {k: [] for k in cases}
        for _ in range(ROUNDS):
            runs = {k: [] for k in cases}
            for _ in range(SAMPLES):
                for k, (g, _) in graphs.items():
                    runs[k].append(sample(g))
            for k in cases:
                medians[k].append(statistics.median(runs[k]))
        for k in cases:
            med = statistics.median(medians[k])
            line = {"tool": "bench_boxes", "shape": [N, 1024, 1024], "case": k, "us": round(med, 2), "rounds_us": [round(v, 2) for v in medians[k]],
                    "spread_us": round(max(medians[k]) - min(medians[k]), 2), "samples": SAMPLES, "replays_per_sample": REPLAYS,
                    "gb_per_s_mask_bytes": round(m.numel() / med / 1e3, 1), "device": torch.cuda.get_device_name(0)}
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
