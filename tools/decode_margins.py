"""The top-2 margin policy of DESIGN 10a, measured: at which bf16 margins does a lossy decode mode pick another token?

    python tools/decode_margins.py [--tokens 64] [--out profiles/decode_margins.jsonl]

A 2-layer decoder at Llama-3-8B and at Phi-3-mini width, SYNTHETIC weights (random, seeded: the logits of such a model are far flatter than a
trained checkpoint's, so the margins are small and flips frequent; the figures bound nothing about a real checkpoint, they show the method).
The bf16 model decodes --tokens tokens greedily with return_scores' records on; every mode — decode_weights = fp8, decode_weights = mxfp4,
kv_cache = fp8, decode_gemv = mfma — then decodes teacher-forced to the bf16 run's ids, so every step sees the same context, and its top1 is
compared with the bf16 top1 of the same step.  Per step: the bf16 margin and the modes whose top1 differs.  Per (width, mode), one JSON line:
the number of flips and the largest bf16 margin at which one was seen (the X of "a token whose bf16 margin exceeds X is expected to be equal in
mode Y" on this model).  There is no CPU path: without a GPU the tool stops."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"fp8": dict(decode_weights="fp8"), "mxfp4": dict(decode_weights="mxfp4"), "kv_cache=fp8": dict(kv_cache="fp8"),
         "decode_gemv=mfma": dict(decode_gemv="mfma")}


def run(llm, tokens):
    import torch
    from videoglamm_amd import synth, vlm
    from videoglamm_amd.params import Params
    device = torch.device("cuda", 0)
    cfg = synth.videoglamm_llama3_8b() if llm == "llama3-8b" else synth.videoglamm_phi3_mini()
    cfg["llm"] = dict(cfg["llm"], num_layers=2)
    man = {k: v for k, v in synth.manifest(cfg).items()
           if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head", "model.text_hidden_fcs"))}
    sd = synth.device_state_dict(man, device, torch.bfloat16)
    g = torch.Generator().manual_seed(11)
    ids = torch.cat([torch.tensor([1, 5, 6, -200, -200, -200, -200]), torch.randint(3, cfg["llm"]["vocab"] - 2, (24,), generator=g)])
    visual = (torch.randn(256, cfg["llm"]["hidden"], generator=g) * 0.5).to(torch.bfloat16).to(device)

    def decode(extra, hook=None):
        c = dict(cfg, llm=dict(cfg["llm"], **extra))
        P = Params(dict(sd), device, torch.bfloat16)          # the mode's own decoder and stored weight forms, the same tensors underneath
        trace = {"scores": True}
        out, _ = vlm.generate(P, c, None, None, None, ids, tokens, None, visual=visual, token_hook=hook, trace=trace)
        return out[ids.numel():].tolist(), trace["scores"]

    base_ids, base = decode({})
    hook = synth.forced_tokens_hook(dict(enumerate(base_ids)))
    flips, lines = {}, []
    for name, extra in MODES.items():
        forced, sc = decode(extra, hook)
        assert forced == base_ids
        flips[name] = sc["top2"][:, 0] != base["top2"][:, 0]
    print(f"# {llm}: step, bf16 top1, bf16 margin, modes whose top1 differs (teacher-forced to the bf16 ids)")
    for j in range(tokens):
        print(f"{j:3d} {int(base['top2'][j, 0]):7d} {float(base['margin'][j]):.6f} " + ",".join(n for n in MODES if flips[n][j]))
    for name in MODES:
        at = base["margin"][flips[name]]
        lines.append(dict(kind="decode_margins", llm=llm, layers=2, weights="synthetic", mode=name, tokens=tokens, flips=int(flips[name].sum()),
                          largest_flip_margin=None if at.size == 0 else round(float(at.max()), 6),
                          median_margin=round(float(sorted(base["margin"])[tokens // 2]), 6)))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("decode_margins: no GPU — the decode modes run on the MI355X kernels only, there is no CPU path")
    torch.set_grad_enabled(False)
    for llm in ("llama3-8b", "phi3-mini"):
        for d in run(llm, args.tokens):
            line = json.dumps(d)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
