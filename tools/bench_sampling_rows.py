"""The B-row sampling launch (vg_sample_partial_rows) against B single-row launches (vg_sample_partial, what RowsDecode._step issued per token
before) at V = 32 064 and 128 256, B = 2, 8, 16, on the fast route (k = 50, p = 0.9, T = 0.6) and the general route (k = 0, p = 0.9).  Each
form is captured 50 times into one graph and replayed; one JSON line per (V, B, route): us per token (all B rows) of either form, median and
minimum of --reps replays.  The rows differ (their own logits, seed and step word), as the rows of a decode step do.

    python tools/bench_sampling_rows.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoglamm_amd import ops  # noqa: E402

N_PER_GRAPH = 50
MODES = {"fast": (0.6, 50, 0.9), "general": (1.0, 0, 0.9)}


def replayed(fn, reps):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        for _ in range(N_PER_GRAPH):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / N_PER_GRAPH)
    times.sort()
    return round(times[len(times) // 2], 2), round(times[0], 2)


def bench(V, B, mode, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(V + B)
    x = (torch.randn(B, V, generator=g) * 3).to(dev)
    T, k, p = MODES[mode]
    params = torch.stack([ops.sampling_params(T, k, p, 1234 + b, dev) for b in range(B)])
    step = torch.arange(B, dtype=torch.int32, device=dev)
    acc = torch.zeros(B, dtype=torch.int64, device=dev)
    ws1 = ops.sample_workspace(dev) if mode == "fast" else None
    wsB = ops.sample_workspace_rows(B, dev) if mode == "fast" else None

    def single():
        for b in range(B):
            ops.sample_partial(x[b], params[b], step[b:b + 1], acc=acc[b:b + 1], fast_ws=ws1)

    def rows():
        ops.sample_partial_rows(x, params, step, acc=acc, fast_ws=wsB)

    single()
    want = acc.clone()
    rows()
    assert torch.equal(acc, want)
    s_med, s_min = replayed(single, reps)
    r_med, r_min = replayed(rows, reps)
    return dict(kind="sample_rows", V=V, B=B, route=mode, single_launches_us=s_med, single_launches_us_min=s_min, rows_launch_us=r_med,
                rows_launch_us_min=r_min, reps=reps, per_graph=N_PER_GRAPH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for V in (32064, 128256):
        for B in (2, 8, 16):
            for mode in MODES:
                line = json.dumps(bench(V, B, mode, args.reps))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
