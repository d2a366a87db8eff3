"""The validator's class counts on the MI355X: the fused call (postproc.validation_counts -> vg_logit_class_counts) against the
torch formula the reference's validator runs per frame, on the same device tensors.
usage: timeout -k 10 600 python tools/bench_validate.py [out.jsonl]      (default: profiles/bench_validate.jsonl, appended)

  A  postproc.validation_counts(logits, gt)            one launch over all frames, eager: what a caller pays, launch included
  A' the same call captured into a graph and replayed   the device time of the memset + kernel; bytes / s is taken from this one
  B  the torch formula                                  threshold, int cast, then per frame: clone, masked assignment, boolean
                                                        gather, three histc, the adds and the division (R/utils/utils.py:78-90,
                                                        R/utils/trainer.py:421, 443-451)

B cannot be captured (the boolean gather sizes its result on the host), so A and B are timed eagerly: a sample is the device-event
time around CALLS calls divided by CALLS, after warm calls; a figure is the median of SAMPLES samples, and the cases alternate
inside each of ROUNDS rounds so that drift hits them alike.  The spread of a case is max - min of its rounds' medians.
Shapes: [1, 30, 360, 640], the validator's own, and [1, 32, 1024, 1024]; logits in fp32 and bf16."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videoglamm_amd import ops, postproc      # noqa: E402

SAMPLES, CALLS, REPLAYS, ROUNDS = 10, 5, 20, 3
HBM_ACHIEVABLE = 6.3e12       # bytes / s, the achievable HBM rate of the MI355X this project measures against


def inputs(shape, seed, dtype, dev):
    """seeded blobby logits (box-filtered noise, zero mean) and a ground truth that follows them loosely, with an ignore band"""
    rng = np.random.RandomState(seed)
    x = rng.rand(*shape).astype(np.float32)
    for ax in (-2, -1):
        for _ in range(4):
            x = (np.roll(x, 1, ax) + x + np.roll(x, -1, ax)) / 3
    x = (x - np.median(x)) * 40
    gt = (np.roll(x, 5, -1) > 0).astype(np.uint8)
    gt[..., :, -8:] = 255
    return torch.from_numpy(x).to(dev, dtype), torch.from_numpy(gt).to(dev)


def torch_formula(logits, gt, ignore_index=255):
    """what the validator computes from one sample's logits [1, T, H, W] and ground truth, as plain torch on the device; returns
    (intersection [2], union [2], acc_iou [2]) device tensors"""
    output = (logits > 0).int()[0]
    target = gt.int()[0]
    intersection = union = acc = 0.0
    for out_t, tgt_t in zip(output, target):
        o, t = out_t.contiguous().clone().view(-1), tgt_t.contiguous().view(-1)
        o[t == ignore_index] = ignore_index
        hit = o[o == t]
        area_i = torch.histc(hit, bins=2, min=0, max=1)
        area_u = torch.histc(o, bins=2, min=0, max=1) + torch.histc(t, bins=2, min=0, max=1) - area_i
        intersection = intersection + area_i
        union = union + area_u
        acc = acc + area_i / (area_u + 1e-5)
        acc[area_u == 0] += 1.0
    return intersection, union, acc


def eager(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3      # us


def replayed(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPLAYS * 1e3      # us


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_validate.jsonl")
    dev = torch.device("cuda:0")
    lines = []
    for shape in ((1, 30, 360, 640), (1, 32, 1024, 1024)):
        for dtype in (torch.float32, torch.bfloat16):
            x, gt = inputs(shape, shape[1], dtype, dev)
            fused = lambda: postproc.validation_counts(x, gt)
            formula = lambda: torch_formula(x, gt)
            # the two sides agree before anything is timed: the formula sums in float32 (inexact past 2^24 pixels, in its own order),
            # which is the arithmetic record_from_counts applies to the exact table
            c = fused()[0].sum(0)
            ri, ru, ra, n = postproc.record_from_counts(fused().cpu().numpy())
            fi, fu, fa = (v.cpu().numpy() for v in formula())
            assert np.array_equal(fi, ri) and np.array_equal(fu, ru) and np.allclose(fa / n, ra, rtol=1e-6, atol=0), "the two sides disagree"
            for _ in range(3):
                fused(), formula()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with ops.graph_capture(g):
                keep = fused()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(keep[0].sum(0), c)
            cases = {"A validation_counts (eager)": lambda: eager(fused), "A' validation_counts (graph replay)": lambda: replayed(g),
                     "B torch formula (eager)": lambda: eager(formula)}
            medians = {k: [] for k in cases}
            for _ in range(ROUNDS):
                runs = {k: [] for k in cases}
                for _ in range(SAMPLES):
                    for k, fn in cases.items():
                        runs[k].append(fn())
                for k in cases:
                    medians[k].append(statistics.median(runs[k]))
            nbytes = x.numel() * (x.element_size() + 1)
            for k in cases:
                med = statistics.median(medians[k])
                line = {"tool": "bench_validate", "shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "case": k, "us": round(med, 2),
                        "rounds_us": [round(v, 2) for v in medians[k]], "spread_us": round(max(medians[k]) - min(medians[k]), 2),
                        "samples": SAMPLES, "calls_per_sample": REPLAYS if "replay" in k else CALLS, "input_bytes": nbytes,
                        "device": torch.cuda.get_device_name(0)}
                if k.startswith("A"):
                    line["tb_per_s_input_bytes"] = round(nbytes / med / 1e6, 3)
                    line["share_of_achievable_hbm"] = round(nbytes / (med * 1e-6) / HBM_ACHIEVABLE, 3)
                lines.append(line)
                print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
