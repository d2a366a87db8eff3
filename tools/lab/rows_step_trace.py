"""Kernel-trace driver of the batched decode step: 8 prompts through prompts.generate_prompts at full Phi-3-mini width (32 layers, bf16 synthetic weights), prefix P = 1700 rows,
then 24 replayed B = 8 batched steps (the dispatches a kernel trace then cuts out: the last 24 steps).
--decode-weights fp8: the step with fp8 decode weights (the MLP and the lm_head on vg_decode_gemv_w8_rows).
--kv-cache fp8: the step on the e4m3 K/V cache (vg_decode_attention_rows_kv8, uint8 prefix and slots)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from videoglamm_amd import synth  # noqa: E402
from videoglamm_amd.params import Params  # noqa: E402
from videoglamm_amd.prompts import generate_prompts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--decode-weights", default="bf16", choices=["bf16", "fp8"])
ap.add_argument("--kv-cache", default="bf16", choices=["bf16", "fp8"])
args = ap.parse_args()
torch.set_grad_enabled(False)


class Towers:
    def __init__(self, v):
        self.v = v

    def encode(self, *a):
        return self.v


dev = torch.device("cuda", 0)
full = synth.videoglamm_phi3_mini()
man = {k: v for k, v in synth.vlm_manifest(full).items()
       if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head", "model.text_hidden_fcs"))}
P = Params(synth.device_state_dict(man, dev, torch.bfloat16), dev, torch.bfloat16)
c = full["llm"] if args.decode_weights == "bf16" else dict(full["llm"], decode_weights="fp8")
if args.kv_cache == "fp8":
    c = dict(c, kv_cache="fp8")
g = torch.Generator().manual_seed(1)
nvis = 1697
visual = (torch.randn(nvis, c["hidden"], generator=g) * 0.5).to(torch.bfloat16).to(dev)
head = torch.tensor([1, 5, 6, -200])
ids = [torch.cat([head, torch.randint(3, c["vocab"] - 2, (30,), generator=g)]) for _ in range(8)]
cfg = dict(llm=c, seg_token_idx=full["seg_token_idx"])
generate_prompts(P, cfg, Towers(visual), None, None, ids, 32)
rows = next(iter(P._decoder._rows.values()))
print(f"row0 {rows.row0} n_bound {rows.n_bound} start_pos {rows.start_pos} B {rows.B} attn_rows {rows.attn_rows} kv_cache {args.kv_cache} "
      f"slot bytes {sum(t.numel() * t.element_size() for t in rows.ks + rows.vs)}", flush=True)
rows.set_positions(rows.start_pos)
rows.decode_step()
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(24):
    rows.decode_step()
torch.cuda.synchronize()
print(f"ms per replayed step: {(time.perf_counter() - t) * 1000 / 24:.3f}", flush=True)
