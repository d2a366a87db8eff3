"""Masks as run-length codes on the MI355X (vg_mask_rle_count / vg_mask_rle_emit / vg_rle_to_mask) against what a caller pays today.
usage: python tools/bench_rle.py [out.jsonl]      (default: profiles/bench_rle.jsonl, appended)

  a  model._to_host(m)                                   the dense download: one DMA into a pinned tensor
  b  model._to_host(m), then the numpy encoder           what a caller who wants codes pays today
  c  ops.mask_rle(m) and its two downloads               the codes leave the device, the masks do not
  d  ops.rle_to_mask(counts, offsets)                    decode, from codes that are on the device
  e  ops.mask_rle(m), the codes stay on the device       the device's share of c (it still reads the 8-byte total)

on 32 x 1024^2 masks, once of blob shapes and once of density 0.5 (the worst case: a run every other pixel, the code is larger than
the mask).  Every case ends with the stream synchronised and is timed on the host clock (downloads and the 8-byte read that sizes the
output are part of what is measured, so nothing here can be replayed from a graph).  A figure is the median of SAMPLES samples; the
cases alternate inside each of ROUNDS rounds, so that drift hits them alike; the spread of a case is max - min of its rounds' medians."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from videoglamm_amd import ops                                  # noqa: E402
from videoglamm_amd.model import VideoGLaMMForCausalLM          # noqa: E402

SAMPLES, ROUNDS = 10, 3
HOST_SAMPLES = 2        # case b runs for seconds at density 0.5


def blobs(shape, seed, density=0.3, grid=12):
    """seeded masks of object-like shape: coarse noise (grid x grid) interpolated up to the mask's size, above a quantile.  A column of a
    1024^2 mask crosses a handful of outlines, so a mask has a few thousand runs, as a segmentation mask has"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape[0], 1, grid, grid, generator=g)
    x = torch.nn.functional.interpolate(x, size=shape[-2:], mode="bicubic", align_corners=False)[:, 0]
    return (x > torch.quantile(x.flatten(1)[:, ::64], 1 - density, dim=1)[:, None, None]).numpy()


def encode_np(mask):
    """the encoder as numpy states it: runs of the column-major pixel order, a leading 0 when pixel 0 is foreground"""
    f = (mask != 0).T.reshape(-1)
    p = np.flatnonzero(f[1:] != f[:-1]) + 1
    return ([0] if f[0] else []) + np.diff(np.concatenate(([0], p, [f.size]))).tolist()


def to_host(m):
    return VideoGLaMMForCausalLM._to_host(None, m)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6      # us


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_rle.jsonl")
    dev = torch.device("cuda:0")
    N, H, W = 32, 1024, 1024
    rng = np.random.default_rng(1)
    sets = {"blobs": blobs((N, H, W), 7), "density 0.5": rng.random((N, H, W)) < 0.5}
    lines = []
    for name, host in sets.items():
        m = torch.from_numpy(host).to(dev).view(torch.uint8)
        counts, offsets = ops.mask_rle(m)
        first = encode_np(host[0])
        assert counts[:int(offsets[1])].tolist() == first, "the device's code of mask 0 is not numpy's"
        back, status = ops.rle_to_mask(counts, offsets, H, W)
        assert not status.any() and torch.equal(back, m), "the round trip changed a mask"
        del back

        def host_encode():
            h = to_host(m).numpy()
            return [encode_np(x) for x in h.reshape(-1, H, W)]

        def device_encode():
            c, o = ops.mask_rle(m)
            return c.cpu(), o.cpu()

        cases = {"a _to_host": lambda: to_host(m), "b _to_host + numpy encoder": host_encode, "c mask_rle + downloads": device_encode,
                 "d rle_to_mask": lambda: ops.rle_to_mask(counts, offsets, H, W), "e mask_rle, codes stay on the device": lambda: ops.mask_rle(m)}
        for fn in cases.values():
            fn()                                # warm: code objects, the allocators (pinned blocks included)
        medians = {k: [] for k in cases}
        for _ in range(ROUNDS):
            runs = {k: [] for k in cases}
            for s in range(SAMPLES):
                for k, fn in cases.items():
                    if k.startswith("b") and s >= HOST_SAMPLES:
                        continue
                    runs[k].append(timed(fn))
            for k in cases:
                medians[k].append(statistics.median(runs[k]))
        for k in cases:
            med = statistics.median(medians[k])
            line = {"tool": "bench_rle", "shape": [N, H, W], "masks": name, "case": k, "us": round(med, 1), "rounds_us": [round(v, 1) for v in medians[k]],
                    "spread_us": round(max(medians[k]) - min(medians[k]), 1), "samples": HOST_SAMPLES if k.startswith("b") else SAMPLES,
                    "runs_total": int(offsets[-1]), "code_bytes": int(offsets[-1]) * 4, "mask_bytes": m.numel(),
                    "device": torch.cuda.get_device_name(0)}
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
