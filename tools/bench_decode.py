"""Decode-loop microbenchmark: Llama-3-8B (synthetic weights), prefill of S random embeddings, then G graph-replayed
decode steps; the 16 GB of weights stream from HBM every token (no MALL flattery as in a single-matrix loop).
usage: python tools/bench_decode.py [S=1697] [G=32] [decode_weights=bf16,fp8,mxfp4] [kv_cache=bf16,fp8,fp8_rope] [llm=llama3-8b|phi3-mini] [reps=3] [out=FILE]
env: VG_DECODE_FUSED=0/1
decode_weights=...: one decoder per mode (cfg["llm"]["decode_weights"]) on the fused kernels, all built, prefilled and captured first; then `reps`
repetitions of G replayed steps per mode, the modes alternating inside every repetition and each repetition starting again at position S.  Per mode:
ms per token of every repetition, their median and spread (max - min).  out=FILE appends the printed lines to FILE.
kv_cache=...: cfg["llm"]["kv_cache"]; with it (and / or decode_weights=) every (decode_weights, kv_cache) pair is one decoder, all alternating;
under kv_cache=fp8 the single-row step is the decode_attention form at either width; kv_cache=fp8_rope is the rope step on e4m3 caches (Llama-3 width only).  llm=phi3-mini: the released checkpoint's LLM (MHA, head_dim 96)."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoglamm_amd import synth  # noqa: E402
from videoglamm_amd.params import Params  # noqa: E402
from videoglamm_amd.vlm import LlamaDecoder  # noqa: E402

pos_args = [a for a in sys.argv[1:] if "=" not in a]
kv_args = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
S = int(pos_args[0]) if len(pos_args) > 0 else 1697
G = int(pos_args[1]) if len(pos_args) > 1 else 32
modes = None
if "decode_weights" in kv_args or "kv_cache" in kv_args:
    modes = [(w, k) for w in kv_args.get("decode_weights", "bf16").split(",") for k in kv_args.get("kv_cache", "bf16").split(",")]
reps = int(kv_args.get("reps", "3"))
dev = torch.device("cuda:0")
cfg = synth.videoglamm_phi3_mini() if kv_args.get("llm") == "phi3-mini" else synth.videoglamm_llama3_8b()
man = {k: v for k, v in synth.vlm_manifest(cfg).items() if k.startswith(("model.layers.", "model.embed_tokens", "model.norm", "lm_head"))}
sd = synth.device_state_dict(man, dev, torch.bfloat16)
P = Params(sd, dev, torch.bfloat16)
llm = cfg["llm"]
nbytes = sum(v.numel() * 2 for k, v in sd.items() if "embed_tokens" not in k)
sync = os.environ.get("BENCH_DECODE_SYNC", "1") == "1"      # 1: read every token back before the next step (the r05 loop); 0: steps back to back


def say(line):
    print(line, flush=True)
    if "out" in kv_args:
        with open(kv_args["out"], "a") as f:
            f.write(line + "\n")


def prefill(c):
    dec = LlamaDecoder(P, c, -(-(S + G + 2) // 1024) * 1024)
    x = (torch.randn(S, llm["hidden"], device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.02).to(torch.bfloat16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = dec.forward(x)
    dec.next_token(h[-1:])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    dec.decode_step()          # eager + capture
    torch.cuda.synchronize()
    return dec, 1e3 * (t1 - t0)


def steps(dec):
    toks = []
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for _ in range(G):
        dec.decode_step()
        if sync:
            toks.append(int(dec.tok_dev[0]))
    torch.cuda.synchronize()
    return (time.perf_counter() - t2) * 1e3 / G, toks


if modes is None:
    for fused in os.environ.get("BENCH_DECODE_FUSED", "0,1").split(","):
        os.environ["VG_DECODE_FUSED"] = fused
        dec, pre = prefill(llm)
        ms, toks = steps(dec)
        say(f"fused={fused} rope_path={dec.rope_path} kpw2={dec.kpw2} sync={int(sync)}: prefill S={S} {pre:.1f} ms; decode {ms:.3f} ms/token "
            f"({nbytes / ms / 1e9:.2f} TB/s of weight bytes); tokens {toks[:8]}")
        del dec
else:
    def mode_cfg(m):
        c = llm if m[0] == "bf16" else dict(llm, decode_weights=m[0])
        return c if m[1] == "bf16" else dict(c, kv_cache=m[1])

    decs = {m: prefill(mode_cfg(m))[0] for m in modes}
    tok0 = {m: d.tok_dev.clone() for m, d in decs.items()}
    times = {m: [] for m in modes}
    first = {}
    for r in range(reps):
        for m in modes:
            d = decs[m]
            d.pos = S + 1                      # every repetition replays the same positions (the captured step reads *pos_dev)
            d.pos_dev.fill_(S + 1)
            d.tok_dev.copy_(tok0[m])
            ms, toks = steps(d)
            times[m].append(ms)
            first.setdefault(m, toks[:8])
    for m in modes:
        t = times[m]
        say(f"decode_weights={m[0]} kv_cache={m[1]} S={S} G={G} sync={int(sync)} rope_path={decs[m].rope_path}: ms/token per repetition {[round(v, 4) for v in t]}, "
            f"median {statistics.median(t):.4f}, spread {max(t) - min(t):.4f}; tokens {first[m]}")
