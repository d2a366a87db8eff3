"""Masks of the fp8 LLM path (fp8 MFMA prefill + fp8 decode weights) against the bf16 path on the full-size synthetic C1
model (Llama-3-8B + towers + SAM2-L, random weights), teacher-forced: the fp8 run is made to emit the ids of the bf16 run, so
the [SEG] hidden states differ by the fp8 arithmetic only.  Prints the cosine of the [SEG] embeddings seen by SAM2 (through the
masks) and the per-mask IoU.  usage: python tools/fp8_mask_iou.py [objects] [--kv-cache fp8|fp8_rope] [--llm llama3-8b|phi3-mini]
--kv-cache fp8: the run compared against bf16 is instead the fp8 K/V cache (cfg["llm"]["kv_cache"] = "fp8"; bf16 weights), teacher-forced
the same way (--kv-cache fp8_rope: the same format on the rope step, Llama-3 width only; the new token there attends to its own K/V quantised);
also printed per step: the relative error and the cosine of the lm_head logits against the bf16 run's, and the argmax agreement.
--llm phi3-mini: the released checkpoint's LLM (MHA, head_dim 96: the model the K/V mode is meant for)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoglamm_amd import synth  # noqa: E402
from videoglamm_amd.model import VideoGLaMMForCausalLM  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("objects", type=int, nargs="?", default=3)
ap.add_argument("--kv-cache", default="bf16", choices=["bf16", "fp8", "fp8_rope"])
ap.add_argument("--llm", default="llama3-8b", choices=["llama3-8b", "phi3-mini"])
args = ap.parse_args()
objects = args.objects
dev = torch.device("cuda:0")
cfg = synth.videoglamm_llama3_8b() if args.llm == "llama3-8b" else synth.videoglamm_phi3_mini()
seg = cfg["seg_token_idx"]
sd = synth.device_state_dict(synth.manifest(cfg), dev, torch.bfloat16)
g = torch.Generator().manual_seed(0)
T, te, S, src, new = 4, 8, 1024, 512, 16
images, context = torch.randn(te, 3, 224, 224, generator=g).to(dev), torch.randn(te, 3, 336, 336, generator=g).to(dev)
sam = torch.randn(T, 3, S, S, generator=g).to(dev)
ids = torch.cat([torch.tensor([1, 5, 6]), torch.full((te,), -200), torch.randint(3, cfg["llm"]["vocab"] - 2, (30,), generator=g)])[None]
forced = {3 + 4 * i: seg for i in range(objects)}
base = synth.install_forced_tokens(VideoGLaMMForCausalLM(sd, dict(cfg, forced_tokens=forced), torch_dtype=torch.bfloat16, device=dev))
out_ids, segs = base.inference([images], [context], [sam], ids, [(S, S)], [(src, src)], max_new_tokens=new)
emitted = out_ids[0, ids.shape[1]:].tolist()
ref = np.stack([np.stack([segs[0][t][k] for k in sorted(segs[0][t])]) for t in sorted(segs[0])])


def step_logits(m):
    """fp32 lm_head logits of the final-norm rows that emitted the tokens (checker arithmetic in torch, outside the product path)"""
    dec = m.P._decoder
    first = dec.pos - len(emitted)                 # the row of the last prompt position
    return dec.hid_all[first:first + len(emitted)].float() @ m.P.t("lm_head.weight").float().t()


ref_logits = step_logits(base)
del base
runs = (("fp8 decode weights", dict(cfg["llm"], decode_weights="fp8")), ("fp8 prefill + decode weights", dict(cfg["llm"], decode_weights="fp8", prefill_gemm="fp8")))
if args.kv_cache != "bf16":
    runs = ((f"fp8 K/V cache ({args.kv_cache})", dict(cfg["llm"], kv_cache=args.kv_cache)),)
for name, llm in runs:
    sd["_"] = None
    sd.pop("_")
    m = synth.install_forced_tokens(VideoGLaMMForCausalLM(sd, dict(cfg, llm=llm, forced_tokens={i: t for i, t in enumerate(emitted)}), torch_dtype=torch.bfloat16, device=dev))
    if hasattr(m.P, "_decoder"):
        del m.P._decoder
    o2, s2 = m.inference([images], [context], [sam], ids, [(S, S)], [(src, src)], max_new_tokens=new)
    assert o2[0].tolist() == out_ids[0].tolist()
    got = np.stack([np.stack([s2[0][t][k] for k in sorted(s2[0][t])]) for t in sorted(s2[0])])
    iou = [[float((got[t, n] & ref[t, n]).sum() / max((got[t, n] | ref[t, n]).sum(), 1)) for n in range(ref.shape[1])] for t in range(T)]
    flat = np.array(iou).ravel()
    print(f"{name}: {ref.shape[1]} objects x {T} frames, mask IoU vs bf16: mean {flat.mean():.4f} median {np.median(flat):.4f} min {flat.min():.4f}")
    print("   per-mask [t][n]:", np.round(np.array(iou), 3).tolist())
    if args.kv_cache != "bf16":
        lg = step_logits(m)
        rel = ((lg - ref_logits).norm(dim=1) / ref_logits.norm(dim=1)).tolist()
        cos = torch.nn.functional.cosine_similarity(lg, ref_logits, dim=1).tolist()
        same = (lg.argmax(1) == ref_logits.argmax(1)).tolist()
        print(f"   lm_head logits vs bf16 per step (step 0 = the prefill's row, unquantised K/V): relative error {[round(v, 5) for v in rel]}")
        print(f"   cosine {[round(v, 6) for v in cos]}")
        print(f"   argmax agreement {sum(same)} of {len(same)} steps: {[int(v) for v in same]}")
    del m
