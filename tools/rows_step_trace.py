"""The replayed batched decode step under rocprofv3 --kernel-trace --stats, and the per-kernel table of its dispatches.

    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/rows_step_trace.py run [--llm llama3-8b] [--batch 16] [--decode-gemv mfma | mfma_q]
                                                                            [--decode-weights fp8 | mxfp4] [--kv-cache fp8 | fp8_rope]
    python tools/rows_step_trace.py table DIR/kt_results.db [--steps 24] > profiles/NAME.txt

run:   clips.generate_clips with --batch clips (a visual block of 1694 rows each, questions of 30..45 ids, 4 new tokens) at the LLM's full depth
       on synthetic bf16 weights, then --steps replayed steps of the batched state (one clip: of the decoder's single-row step); prints the wall
       time per replayed step.
table: the dispatches of the last --steps steps of the trace (a step starts at its decode_step_begin kernel), per kernel, grid and place in the
       layer: dispatches per step, us per dispatch, us per step, share.  Two projections of one template instance and grid (o and down at Llama
       width) are told apart by their order inside the layer."""
import argparse
import collections
import os
import sqlite3
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(args):
    import torch
    from videoglamm_amd import clips, synth, vlm
    from videoglamm_amd.params import Params
    torch.set_grad_enabled(False)
    device = torch.device("cuda", 0)
    cfg = synth.videoglamm_llama3_8b() if args.llm == "llama3-8b" else synth.videoglamm_phi3_mini()
    if args.decode_gemv != "valu":
        cfg["llm"] = dict(cfg["llm"], decode_gemv=args.decode_gemv)
    if args.decode_weights != "bf16":
        cfg["llm"] = dict(cfg["llm"], decode_weights=args.decode_weights)
    if args.kv_cache != "bf16":
        cfg["llm"] = dict(cfg["llm"], kv_cache=args.kv_cache)
    man = {k: v for k, v in synth.manifest(cfg).items() if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head", "model.text_hidden_fcs"))}
    P = Params(synth.device_state_dict(man, device, torch.bfloat16), device, torch.bfloat16)
    g = torch.Generator().manual_seed(7)
    head = torch.tensor([1, 5, 6, -200, -200, -200, -200])
    text = [(None, None, torch.cat([head, torch.randint(3, cfg["llm"]["vocab"] - 2, (30 + b,), generator=g)])) for b in range(args.batch)]
    visuals = [(torch.randn(1694, cfg["llm"]["hidden"], generator=g) * 0.5).to(torch.bfloat16).to(device) for _ in range(args.batch)]
    if args.batch == 1:
        vlm.generate(P, cfg, None, None, None, text[0][2], 4, None, visual=visuals[0])
        step = P._decoder.decode_step
    else:
        clips.generate_clips(P, cfg, None, text, 4, None, visuals=visuals)
        rows = next(iter(P._decoder._rows.values()))
        rows.set_positions(rows.start_pos)
        step = rows.decode_step
    step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    print(f"llm {args.llm} decode_gemv {args.decode_gemv} decode_weights {args.decode_weights} kv_cache {args.kv_cache} batch {args.batch}: {(time.perf_counter() - t) * 1000.0 / args.steps:.3f} ms per replayed step "
          f"({args.steps} steps)", flush=True)


def table(args):
    db = sqlite3.connect(args.db)
    rows = list(db.execute("select name, grid_x, grid_y, grid_z, start, end from kernels order by start"))
    begins = [i for i, r in enumerate(rows) if "decode_step_begin" in r[0]]
    assert len(begins) >= args.steps, f"{len(begins)} steps in the trace"
    cut = begins[-args.steps:] + [len(rows)]
    per_step = collections.Counter()
    for a, b in zip(cut[:-1], cut[1:]):
        per_step[b - a] += 1
    n = per_step.most_common(1)[0][0]               # (the last step may drag the end-of-run copies along: cut every step to the common length)
    stat = collections.OrderedDict()
    wall = 0.0
    for a in cut[:-1]:
        seg = rows[a:a + n]
        wall += (seg[-1][5] - seg[0][4]) / 1e3
        seen = collections.Counter()
        for name, gx, gy, gz, s, e in seg:
            seen[(name, gx, gy, gz)] += 1
        occ = collections.Counter()
        for name, gx, gy, gz, s, e in seg:
            k = (name, gx, gy, gz)
            m = seen[k] // args.layers if seen[k] % args.layers == 0 and seen[k] > args.layers else 1
            key = k + (occ[k] % m,)
            occ[k] += 1
            d = stat.setdefault(key, [0, 0.0])
            d[0] += 1
            d[1] += (e - s) / 1e3
    total = sum(d[1] for d in stat.values()) / args.steps
    print(f"# dispatches of the last {args.steps} replayed steps; first dispatch to last dispatch per step = {wall / args.steps / 1e3:.3f} ms; "
          f"sum of kernel times per step = {total / 1e3:.3f} ms")
    print("kernel | grid (x,y,z) | place in the layer | dispatches per step | us per dispatch | us per step | share")
    for (name, gx, gy, gz, j), (cnt, us) in sorted(stat.items(), key=lambda kv: -kv[1][1]):
        print(f"{name} | ({gx},{gy},{gz}) | {j} | {cnt // args.steps} | {us / cnt:.1f} | {us / args.steps:.1f} | {us / args.steps / total:.3f}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--llm", default="llama3-8b", choices=["llama3-8b", "phi3-mini"])
    r.add_argument("--batch", type=int, default=16)
    r.add_argument("--decode-gemv", default="valu", choices=["valu", "mfma", "mfma_q"])
    r.add_argument("--decode-weights", default="bf16", choices=["bf16", "fp8", "mxfp4"], help="mfma_q pairs with fp8 / mxfp4, mfma with bf16")
    r.add_argument("--kv-cache", default="bf16", choices=["bf16", "fp8", "fp8_rope"], help="cfg['llm']['kv_cache'] (DESIGN 8c)")
    r.add_argument("--steps", type=int, default=24)
    t = sub.add_parser("table")
    t.add_argument("db")
    t.add_argument("--steps", type=int, default=24)
    t.add_argument("--layers", type=int, default=32)
    args = ap.parse_args()
    run(args) if args.cmd == "run" else table(args)


if __name__ == "__main__":
    main()
