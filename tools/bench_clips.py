"""Several clips, one prompt each: model.inference_clips() against the same clips as a loop of inference() calls.

Workload: BASELINE config C2 (synthetic Llama-3-8B, 16 encoder frames, 32 x 1024^2 SAM frames, 32 new tokens, [SEG] forced at step 8 as
bench.py does) x B, and the same with the Phi-3-mini LLM (--llm); the B entries are the same clip with B different questions (30 ids).
The two forms alternate inside each repetition; one JSON line per (LLM, mode):
  "clips_ms"[B] / "loop_ms"[B]:  median ms of one inference_clips() call with B clips / of the B inference() calls, over --reps repetitions
  "clips_spread"[B] / "loop_spread"[B]: [min, max] of the repetitions
  "clips_ms_per_clip"[B] / "loop_ms_per_clip"[B]: the medians / B
  "rows_step_ms"[B]:  one replayed batched decode step of the bucket B runs in (vlm.RowsDecode with row0 = 0), rows at the clips' positions
  "decode_step_ms":   one replayed single-row decode step (LlamaDecoder.decode_step), ms per token
--sample k50 / k0: sampled decoding (k 50, p 0.9, T 0.6: the fast route; k 0, p 0.9: the general route), seeded per repetition.
--decode-gemv valu mfma: the decode mode cfg["llm"]["decode_gemv"]; given both, one model per mode is built on the same weights and
the modes alternate inside each repetition (loop, clips and the replayed step of one mode, then of the other); one line per mode, with
"rows_step_spread"[B] / "decode_step_spread" = [min, max] over the repetitions.  mfma_q is the mode of the fp8 / mxfp4 decode weights.
--decode-weights bf16 fp8 mxfp4: cfg["llm"]["decode_weights"]; every valid (decode_gemv, decode_weights) pair is one model and one line
("decode_weights" in the record), all alternating inside each repetition; an invalid pair (mfma with fp8 / mxfp4, mfma_q with bf16) is skipped
with a printed line.
--kv-cache bf16 fp8 fp8_rope: cfg["llm"]["kv_cache"] (fp8_rope at Llama-3 width only); each value is one more model per pair ("kv_cache" in the record), alternating with the
others inside each repetition.  "slot_bytes"[B]: the bytes of the batched state's K / V slots (RowsDecode.ks + vs) behind that B.
--out FILE also appends the lines to FILE (the raw record behind DESIGN 12's table lives in profiles/).

    python tools/bench_clips.py [--llm llama3-8b phi3-mini] [--batches 1 2 4 8 16] [--reps 3] [--warmup 1] [--branch framewise]
                                 [--sample k50 k0] [--decode-gemv valu mfma mfma_q] [--decode-weights bf16 fp8 mxfp4]
                                 [--kv-cache bf16 fp8 fp8_rope] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoglamm_amd import synth  # noqa: E402
from videoglamm_amd.model import VideoGLaMMForCausalLM  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_prompts import decode_step_ms, rows_step_ms  # noqa: E402

SAMPLING = {"greedy": {}, "k50": dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.6), "k0": dict(do_sample=True, top_k=0, top_p=0.9, temperature=1.0)}


def once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000.0


def pairs(args):
    """the valid (decode_gemv, decode_weights) pairs of the two option lists: mfma streams bf16 weights, mfma_q fp8 / mxfp4 (vlm.decode_gemv_mode)"""
    return [(dg, dw, kv) for dw in args.decode_weights for dg in args.decode_gemv for kv in args.kv_cache
            if not (dg == "mfma" and dw != "bf16") and not (dg == "mfma_q" and dw == "bf16")]


def slot_bytes(model):
    """bytes of the K / V slots of the batched state the last inference_clips() call decoded on (None: it ran the plain loop)"""
    rows = getattr(getattr(model.P, "_decoder", None), "_rows", None)
    if not rows:
        return None
    r = next(iter(rows.values()))
    return sum(t.numel() * t.element_size() for t in r.ks + r.vs)


def run(llm, mode, args, device):
    cfg = synth.videoglamm_llama3_8b() if llm == "llama3-8b" else synth.videoglamm_phi3_mini()
    cfg["forced_tokens"] = {8: cfg["seg_token_idx"]}
    sd = synth.device_state_dict(synth.manifest(cfg), device, torch.bfloat16)
    models = {}
    for dg, dw, kv in pairs(args):       # one model per (decode mode, decode weights, K/V cache) on the same weight tensors
        extra = dict(decode_gemv=dg) if dg != "valu" else {}
        if dw != "bf16":
            extra["decode_weights"] = dw
        if kv != "bf16":
            extra["kv_cache"] = kv
        c = dict(cfg, llm=dict(cfg["llm"], **extra)) if extra else cfg
        models[(dg, dw, kv)] = synth.install_forced_tokens(VideoGLaMMForCausalLM(sd, c, torch_dtype=torch.bfloat16, device=device))
    g = torch.Generator().manual_seed(1234)
    te, S = 16, cfg["sam2"]["image_size"]
    iv, cl = cfg["iv2"]["img_size"], cfg["clip"]["img_size"]
    images = [torch.randn(te, 3, iv, iv, generator=g).to(device)]
    context = [torch.randn(te, 3, cl, cl, generator=g).to(device)]
    sam = [torch.randn(args.frames, 3, S, S, generator=g).to(device)]
    head = torch.cat([torch.tensor([1, 5, 6]), torch.full((te,), -200)])
    prompts = [torch.cat([head, torch.randint(3, cfg["llm"]["vocab"] - 2, (30,), generator=g)]) for _ in range(max(args.batches))]
    rest = ([(1024, 1024)], [(args.src, args.src)])
    video = args.branch == "video"
    kw = dict(max_new_tokens=args.max_new_tokens, use_sam2_video_branch=video, **SAMPLING[mode])
    recs = {dg: dict(llm=llm, mode=mode, decode_gemv=dg[0], decode_weights=dg[1], kv_cache=dg[2], branch=args.branch, frames=args.frames, max_new_tokens=args.max_new_tokens, reps=args.reps,
                     clips_ms={}, loop_ms={}, clips_spread={}, loop_spread={}, clips_ms_per_clip={}, loop_ms_per_clip={}, rows_step_ms={},
                     rows_step_spread={}, slot_bytes={}) for dg in models}
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]              # noqa: E731
    for B in args.batches:
        clips = [(images, context, sam, x[None], *rest) for x in prompts[:B]]
        tl, tb, ts = ({dg: [] for dg in models} for _ in range(3))
        for r in range(args.warmup + args.reps):
            for dg, model in models.items():      # the modes alternate inside the repetition
                torch.manual_seed(100 + r)
                a = once(lambda: [model.inference(*c, **kw) for c in clips])
                torch.manual_seed(100 + r)
                b = once(lambda: model.inference_clips(clips, **kw))
                st = rows_step_ms(model) if B > 1 else None
                recs[dg]["slot_bytes"][B] = slot_bytes(model) if B > 1 else None
                if r >= args.warmup:
                    tl[dg].append(a)
                    tb[dg].append(b)
                    ts[dg].append(st)
        for dg, rec in recs.items():
            ml, mb = statistics.median(tl[dg]), statistics.median(tb[dg])
            rec["loop_ms"][B], rec["clips_ms"][B] = round(ml, 2), round(mb, 2)
            rec["loop_spread"][B], rec["clips_spread"][B] = spread(tl[dg]), spread(tb[dg])
            rec["loop_ms_per_clip"][B], rec["clips_ms_per_clip"][B] = round(ml / B, 2), round(mb / B, 2)
            live = [v for v in ts[dg] if v is not None]
            rec["rows_step_ms"][B] = round(statistics.median(live), 4) if live else None
            rec["rows_step_spread"][B] = spread(live) if live else None
    td = {dg: [] for dg in models}
    for r in range(args.reps):
        for dg, model in models.items():
            td[dg].append(decode_step_ms(model, tokens=24))
    for dg, rec in recs.items():
        live = [v for v in td[dg] if v is not None]
        rec["decode_step_ms"] = round(statistics.median(live), 4) if live else None
        rec["decode_step_spread"] = spread(live) if live else None
    del models, sd
    torch.cuda.empty_cache()
    return list(recs.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--llm", nargs="+", default=["llama3-8b", "phi3-mini"], choices=["llama3-8b", "phi3-mini"])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions (>= 3 for a median and a spread)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--src", type=int, default=1024)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--branch", default="framewise", choices=["framewise", "video"])
    ap.add_argument("--sample", nargs="*", default=None, choices=["k50", "k0"], help="also (or, given alone with --no-greedy, only) the sampled modes")
    ap.add_argument("--no-greedy", action="store_true")
    ap.add_argument("--decode-gemv", nargs="+", default=["valu"], choices=["valu", "mfma", "mfma_q"],
                    help="cfg['llm']['decode_gemv']; several: the modes alternate inside each repetition, one line per mode")
    ap.add_argument("--decode-weights", nargs="+", default=["bf16"], choices=["bf16", "fp8", "mxfp4"],
                    help="cfg['llm']['decode_weights']; every valid pair with --decode-gemv is one model, invalid pairs are skipped")
    ap.add_argument("--kv-cache", nargs="+", default=["bf16"], choices=["bf16", "fp8", "fp8_rope"],
                    help="cfg['llm']['kv_cache']; each value is one more model per (decode_gemv, decode_weights) pair")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    device = torch.device("cuda", 0)
    modes = ([] if args.no_greedy else ["greedy"]) + list(args.sample or [])
    for dw in args.decode_weights:
        for dg in args.decode_gemv:
            if (dg, dw, args.kv_cache[0]) not in pairs(args):
                print(f"# skipped: decode_gemv = {dg} does not combine with decode_weights = {dw}", flush=True)
    for llm in args.llm:
        for mode in modes:
            for rec in run(llm, mode, args, device):
                line = json.dumps(rec)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
