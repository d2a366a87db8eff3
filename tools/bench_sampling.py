"""Cost of sampled decoding per token at the Llama-3 (V = 128 256, hidden 4096) and Phi-3 (V = 32 064, hidden 3072) widths: greedy
(vg_argmax_partial) against the sampler's fast route (k = 50, p = 0.9, T = 0.6: 64 workgroups + last-arriver merge) and general route
(k = 0, p = 0.9: one workgroup, every pass reads the row).  Two measurements, one JSON line each per (width, mode):
  "launch": the token-selection launch alone, captured 200 times into one graph and replayed (us per token);
  "step":   a whole replayed decode step (LlamaDecoder.decode_step: embed, the layers, lm_head, token selection, tail) of a decoder with
            --layers layers at that width (random weights), ms per token over --tokens replays.
Kernel times for the same launches: run under rocprofv3 --kernel-trace --stats in a separate run.

    python tools/bench_sampling.py [--reps 20] [--layers 4] [--tokens 200]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoglamm_amd import ops  # noqa: E402

N_PER_GRAPH = 200
MODES = {"greedy": None, "fast": (0.6, 50, 0.9), "general": (1.0, 0, 0.9)}
WIDTHS = {"llama3": dict(vocab=128256, hidden=4096, ffn=14336, num_heads=32, num_kv_heads=8, rms_eps=1e-5, rope_theta=500000.0),
          "phi3": dict(vocab=32064, hidden=3072, ffn=8192, num_heads=32, num_kv_heads=32, rms_eps=1e-5, rope_theta=10000.0, sliding_window=2047,
                       fused_proj=True)}


def bench(V, mode, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(V)
    x = (torch.randn(V, generator=g) * 3).to(dev)
    acc = torch.zeros(1, dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    params = ops.sampling_params(*MODES[mode], 1234, dev) if MODES[mode] else None
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = ops.sample_workspace(dev) if mode == "fast" else None

    def one():
        if mode == "greedy":
            ops.argmax_partial(x, acc)
        else:
            ops.sample_partial(x, params, step, acc=acc, fast_ws=ws)
        acc.copy_(zero)          # the consumer's reset (vg_decode_step_end leaves it zero); the same in every mode

    one()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        for _ in range(N_PER_GRAPH):
            one()
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
    return dict(kind="launch", V=V, mode=mode, us_per_token_median=round(times[len(times) // 2], 2), us_per_token_min=round(times[0], 2), reps=reps,
                launches_per_graph=N_PER_GRAPH)


def bench_step(width, layers, tokens, prompt=1024):
    """one decoder per width; every mode replays its own captured step from the same KV cache state"""
    from videoglamm_amd import synth
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    dev = torch.device("cuda")
    c = dict(WIDTHS[width], num_layers=layers)
    cfg = dict(synth.videoglamm_llama3_8b(), llm=c, seg_token_idx=c["vocab"] - 1)
    man = {k: v for k, v in synth.vlm_manifest(cfg).items() if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))}
    P = Params(synth.device_state_dict(man, dev, torch.bfloat16, seed=1), dev, torch.bfloat16)
    dec = LlamaDecoder(P, c, prompt + tokens + 64)
    x = torch.randn(prompt, c["hidden"], device=dev).mul_(0.5).to(torch.bfloat16)
    dec.forward(x)
    out = []
    for mode, prm in MODES.items():
        dec.set_sampling(None if prm is None else dict(T=prm[0], k=prm[1], p=prm[2], seed=1234))
        dec.pos = prompt
        dec.pos_dev.fill_(prompt)
        dec.step_dev.fill_(1)
        dec.decode_step()                  # capture
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dec.pos = prompt
        dec.pos_dev.fill_(prompt)
        e0.record()
        for _ in range(tokens):
            dec.decode_step()
        e1.record()
        e1.synchronize()
        out.append(dict(kind="step", width=width, V=c["vocab"], layers=layers, mode=mode, route=dec.samp_fast if prm else None,
                        ms_per_token=round(e0.elapsed_time(e1) / tokens, 4), tokens=tokens))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=200)
    ap.add_argument("--launch-only", action="store_true")
    args = ap.parse_args()
    for V in (128256, 32064):
        for mode in MODES:
            print(json.dumps(bench(V, mode, args.reps)), flush=True)
    if not args.launch_only:
        for width in WIDTHS:
            for r in bench_step(width, args.layers, args.tokens):
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
