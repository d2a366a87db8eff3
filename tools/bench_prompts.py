"""Several prompts about one clip: model.inference_prompts() against the same prompts as sequential inference() calls.

Workload: BASELINE config C2 (synthetic Llama-3-8B, 16 encoder frames, 32 x 1024^2 SAM frames, 32 new tokens, [SEG] forced at step 8 as
bench.py does) and the same clip with the Phi-3-mini LLM (--llm).  The prompts share bench.py's prefix ([1, 5, 6] + the visual block) and
differ in their 30 question ids.  One JSON line per LLM:
  "prompts_ms"[B]:    ms per inference_prompts() call with B prompts
  "sequential_ms"[B]: ms for the same B prompts as B inference() calls
  "ratio"[B]:         prompts_ms / sequential_ms
  "decode_step_ms":   one replayed decode step of one prompt (LlamaDecoder.decode_step, the step the sequential loop decodes with), ms per token
  "rows_step_ms"[B]:  one replayed batched decode step of the bucket B runs in (vlm.RowsDecode: Llama-3 and Phi-3-mini widths), ms per step
--decode-weights fp8 / --prefill fp8: the fp8 LLM path (bench.py's switches of the same names), written into each line.
--ab also times inference_prompts() with VG_PROMPTS_BATCHED=0 ("prompts_seq_ms"[B]: the prompts decoded one after another).
--shared passes shared=True: the shared route for every model.  An mxfp4 model takes it only then (its default is one inference() per prompt, which
is what "sequential_ms" times), so --decode-weights mxfp4 --shared --ab compares the batched MXFP4 step with the sequential loop on that route.
--decode-gemv mfma / mfma_q: the decode modes cfg["llm"]["decode_gemv"] = "mfma" (bf16 decode weights only) / "mfma_q" (fp8 / mxfp4 only), written into each line; given both values, one
line per mode, each LLM's two runs back to back.
--out FILE also appends the lines to FILE (the raw record behind DESIGN 11's table lives in profiles/).

    python tools/bench_prompts.py [--llm llama3-8b phi3-mini] [--batches 1 2 4 8] [--steps 3] [--warmup 1] [--branch framewise]
                                   [--decode-weights fp8|mxfp4] [--prefill fp8] [--shared] [--ab] [--decode-gemv valu mfma mfma_q]
                                   [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoglamm_amd import synth  # noqa: E402
from videoglamm_amd.model import VideoGLaMMForCausalLM  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000.0 / steps


def decode_step_ms(model, tokens=64):
    """replayed decode steps of the cached decoder, continuing from where the last call left it (rows past the clip: scratch)"""
    dec = model.P._decoder
    tokens = min(tokens, dec.max_len - dec.pos - 3)
    if tokens < 2:
        return None
    for _ in range(2):                 # settle (and capture, should this position range need a graph of its own)
        dec.decode_step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(tokens - 1):
        dec.decode_step()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) / (tokens - 1), 4)


def rows_step_ms(model, tokens=32):
    """replayed steps of the batched state the last inference_prompts() call left, every row restarted at the position it was loaded at (the end
    of its suffix): the steps attend as many keys as the first steps of the real loop and overwrite only that loop's own decode rows"""
    rows = next(iter(getattr(model.P._decoder, "_rows", {}).values()), None)
    if rows is None:
        return None
    tokens = min(tokens, rows.n_bound - max(rows.start_pos) - 2)
    rows.set_positions(rows.start_pos)
    for _ in range(2):
        rows.decode_step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(tokens - 1):
        rows.decode_step()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) / (tokens - 1), 4)


def run(llm, args, device, decode_gemv="valu"):
    cfg = synth.videoglamm_llama3_8b() if llm == "llama3-8b" else synth.videoglamm_phi3_mini()
    cfg["forced_tokens"] = {8: cfg["seg_token_idx"]}
    if decode_gemv != "valu":
        cfg["llm"] = dict(cfg["llm"], decode_gemv=decode_gemv)
    if args.decode_weights in ("fp8", "mxfp4"):
        cfg["llm"] = dict(cfg["llm"], decode_weights=args.decode_weights)
    if args.prefill == "fp8":
        cfg["llm"] = dict(cfg["llm"], prefill_gemm="fp8")
    sd = synth.device_state_dict(synth.manifest(cfg), device, torch.bfloat16)
    model = synth.install_forced_tokens(VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.bfloat16, device=device))
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
    rec = dict(llm=llm, decode_gemv=decode_gemv, decode_weights=args.decode_weights, prefill=args.prefill, branch=args.branch, frames=args.frames,
               max_new_tokens=args.max_new_tokens, shared=args.shared, prompts_ms={}, sequential_ms={}, ratio={},
               rows_step_ms={})
    kw = dict(shared=True) if args.shared else {}
    if args.ab:
        rec["prompts_seq_ms"] = {}
    for B in args.batches:
        P = prompts[:B]
        seq = timed(lambda: [model.inference(images, context, sam, x[None], *rest, args.max_new_tokens, video) for x in P], args.steps, args.warmup)
        bat = timed(lambda: model.inference_prompts(images, context, sam, P, *rest, args.max_new_tokens, video, **kw), args.steps, args.warmup)
        rec["prompts_ms"][B], rec["sequential_ms"][B], rec["ratio"][B] = round(bat, 2), round(seq, 2), round(bat / seq, 3)
        rec["rows_step_ms"][B] = rows_step_ms(model) if B > 1 else None
        if args.ab:
            os.environ["VG_PROMPTS_BATCHED"] = "0"
            try:
                rec["prompts_seq_ms"][B] = round(timed(lambda: model.inference_prompts(images, context, sam, P, *rest, args.max_new_tokens, video,
                                                                                       **kw), args.steps, args.warmup), 2)
            finally:
                os.environ.pop("VG_PROMPTS_BATCHED")
    rec["decode_step_ms"] = decode_step_ms(model)
    del model, sd
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--llm", nargs="+", default=["llama3-8b", "phi3-mini"], choices=["llama3-8b", "phi3-mini"])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--src", type=int, default=1024)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--branch", default="framewise", choices=["framewise", "video"])
    ap.add_argument("--decode-weights", default="bf16", choices=["bf16", "fp8", "mxfp4"],
                    help="fp8: the decode step's MLP and lm_head weights in fp8 (e4m3, row scales), as bench.py --decode-weights; mxfp4: the MLP in MXFP4, "
                         "the lm_head in fp8 (by default inference_prompts() runs such a model's prompts as one inference() each; --shared sends it down "
                         "the shared route, where the prompts decode on the B-row MXFP4 GEMV)")
    ap.add_argument("--prefill", default="bf16", choices=["bf16", "fp8"], help="fp8: the LLM prefill GEMMs on the fp8 MFMA path, as bench.py --prefill")
    ap.add_argument("--shared", action="store_true", help="call inference_prompts(..., shared=True): the shared route for every model, mxfp4 included")
    ap.add_argument("--ab", action="store_true", help="also time inference_prompts() on the sequential loop (VG_PROMPTS_BATCHED=0)")
    ap.add_argument("--decode-gemv", nargs="+", default=["valu"], choices=["valu", "mfma", "mfma_q"],
                    help="cfg['llm']['decode_gemv']; one line per value (mfma: bf16 decode weights only; mfma_q: fp8 / mxfp4 only; an invalid pair "
                         "with --decode-weights is skipped with a printed line)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    device = torch.device("cuda", 0)
    for llm in args.llm:
        for dg in args.decode_gemv:
            if (dg == "mfma" and args.decode_weights != "bf16") or (dg == "mfma_q" and args.decode_weights == "bf16"):
                print(f"# skipped: decode_gemv = {dg} does not combine with decode_weights = {args.decode_weights}", flush=True)
                continue
            line = json.dumps(run(llm, args, device, dg))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
