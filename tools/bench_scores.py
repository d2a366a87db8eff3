"""What return_scores costs on the MI355X: the vg_token_scores_rows launch alone against the greedy argmax launch of the same
build, and a whole replayed decode step of a 4-layer decoder with and without the scores launch.

    python tools/bench_scores.py [--reps 9] [--out profiles/bench_scores.jsonl] [--skip-step]

launch: V = 32 064 and 128 256, B = 1, 8, 16; either launch is captured 50 times into one graph; the two graphs are replayed alternately
        --reps times; us per launch, median and (min, max) of the replays.
step:   synthetic bf16 weights, 4 layers, Phi-3-mini width (V = 32 064) and Llama-3-8B width (V = 128 256), a visual block of 1694 rows;
        B = 1 is the decoder's single-row step, B = 8 / 16 the batched step of clips.generate_clips; the graph without and the graph with
        the scores launch are replayed alternately, 24 steps from the same positions each time; ms per step, median and (min, max).
One JSON line per measurement.  There is no CPU path: without a GPU the tool stops."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_PER_GRAPH = 50
STEPS = 24


def _stats(v, nd):
    v = sorted(v)
    return round(v[len(v) // 2], nd), round(v[0], nd), round(v[-1], nd)


def _graph(fn):
    import torch
    from videoglamm_amd import ops
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        for _ in range(N_PER_GRAPH):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _alternate(graphs, reps):
    """every graph replayed once per repetition, in turn -> us per captured launch, per graph"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = [[] for _ in graphs]
    for _ in range(reps):
        for t, g in zip(times, graphs):
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / N_PER_GRAPH)
    return times


def bench_launch(V, B, reps):
    import torch
    from videoglamm_amd import ops
    dev = torch.device("cuda")
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(V + B)) * 3).to(dev)
    acc = torch.zeros(B, dtype=torch.int64, device=dev)
    step = torch.arange(B, dtype=torch.int32, device=dev)
    scores = torch.zeros(B, 64, 2, dtype=torch.float32, device=dev)
    top2 = torch.zeros(B, 64, 2, dtype=torch.int64, device=dev)
    ws = ops.token_scores_workspace(B, dev)
    ops.argmax_partial_rows(x, acc)          # the key the scores launch reads, as in the step

    def argmax():
        ops.argmax_partial_rows(x, acc)

    def score():
        ops.token_scores_rows(x, step, scores, top2, acc=acc, ws=ws)

    score()
    assert top2[:, :, 0].sum(1).tolist() == x.argmax(1).tolist()
    ta, ts = _alternate([_graph(argmax), _graph(score)], reps)
    (am, alo, ahi), (sm, slo, shi) = _stats(ta, 2), _stats(ts, 2)
    return dict(kind="scores_launch", V=V, B=B, argmax_us=am, argmax_us_min=alo, argmax_us_max=ahi, scores_us=sm, scores_us_min=slo,
                scores_us_max=shi, reps=reps, per_graph=N_PER_GRAPH)


def bench_step(llm, B, reps):
    import torch
    from videoglamm_amd import clips, synth, vlm
    from videoglamm_amd.params import Params
    device = torch.device("cuda", 0)
    cfg = synth.videoglamm_llama3_8b() if llm == "llama3-8b" else synth.videoglamm_phi3_mini()
    cfg["llm"] = dict(cfg["llm"], num_layers=4)
    man = {k: v for k, v in synth.manifest(cfg).items()
           if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head", "model.text_hidden_fcs"))}
    P = Params(synth.device_state_dict(man, device, torch.bfloat16), device, torch.bfloat16)
    g = torch.Generator().manual_seed(7)
    head = torch.tensor([1, 5, 6, -200, -200, -200, -200])
    text = [(None, None, torch.cat([head, torch.randint(3, cfg["llm"]["vocab"] - 2, (30 + b,), generator=g)])) for b in range(B)]
    visuals = [(torch.randn(1694, cfg["llm"]["hidden"], generator=g) * 0.5).to(torch.bfloat16).to(device) for _ in range(B)]
    for on in (False, True):                 # both graphs are captured by the product's own loops
        traces = [{"scores": True} if on else {} for _ in range(B)]
        if B == 1:
            vlm.generate(P, cfg, None, None, None, text[0][2], 4, None, visual=visuals[0], trace=traces[0])
        else:
            clips.generate_clips(P, cfg, None, text, 4, None, visuals=visuals, traces=traces)
    dec = P._decoder
    state = dec if B == 1 else next(iter(dec._rows.values()))
    assert len(state.graphs) == 2, list(state.graphs)
    pos0 = dec.pos if B == 1 else list(state.start_pos)

    def block(on):
        state.set_scores(on)
        if B == 1:
            dec.pos = pos0
            dec.pos_dev.fill_(pos0)
            dec.step_dev.fill_(1)
        else:
            state.set_positions(pos0)
            state.step.fill_(1)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(STEPS):
            state.decode_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1000.0 / STEPS

    block(False), block(True)
    off, on = [], []
    for _ in range(reps):
        off.append(block(False))
        on.append(block(True))
    (om, olo, ohi), (sm, slo, shi) = _stats(off, 4), _stats(on, 4)
    return dict(kind="scores_step", llm=llm, layers=4, V=cfg["llm"]["vocab"], B=B, step_ms=om, step_ms_min=olo, step_ms_max=ohi, step_scores_ms=sm,
                step_scores_ms_min=slo, step_scores_ms_max=shi, reps=reps, steps=STEPS)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--skip-step", action="store_true", help="the launch alone, not the decode step")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scores: no GPU — the measurement runs on the MI355X kernels only, there is no CPU path")
    torch.set_grad_enabled(False)

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for V in (32064, 128256):
        for B in (1, 8, 16):
            emit(bench_launch(V, B, args.reps))
    if not args.skip_step:
        for llm in ("phi3-mini", "llama3-8b"):
            for B in (1, 8, 16):
                emit(bench_step(llm, B, args.reps))


if __name__ == "__main__":
    main()
