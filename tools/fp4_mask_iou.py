"""Masks and logits of MXFP4 decode weights (cfg["llm"]["decode_weights"] = "mxfp4"), and of the MXFP4 prefill on top of them (prefill_gemm = "mxfp4"),
against the bf16 path on the full-size synthetic C1 model
(Llama-3-8B + towers + SAM2-L, random weights) — tools/fp8_mask_iou.py's clip and teacher forcing: the mxfp4 run is made to emit the ids of the bf16
run, so both see the same sequence.  Prints, as DESIGN section 8 quotes them for fp8: relative error and cosine of the lm_head logits per step (formed
here from the final-norm rows and the bf16 lm_head), argmax agreement on the free steps, cosine of the [SEG] embeddings, mask IoU mean / min.
usage: python tools/fp4_mask_iou.py [objects]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoglamm_amd import synth, vlm  # noqa: E402
from videoglamm_amd.model import VideoGLaMMForCausalLM  # noqa: E402

torch.set_grad_enabled(False)
objects = int(sys.argv[1]) if len(sys.argv) > 1 else 3
dev = torch.device("cuda:0")
cfg = synth.videoglamm_llama3_8b()
seg = cfg["seg_token_idx"]
sd = synth.device_state_dict(synth.manifest(cfg), dev, torch.bfloat16)
g = torch.Generator().manual_seed(0)
T, te, S, src, new = 4, 8, 1024, 512, 16
images, context = torch.randn(te, 3, 224, 224, generator=g).to(dev), torch.randn(te, 3, 336, 336, generator=g).to(dev)
sam = torch.randn(T, 3, S, S, generator=g).to(dev)
ids = torch.cat([torch.tensor([1, 5, 6]), torch.full((te,), -200), torch.randint(3, cfg["llm"]["vocab"] - 2, (30,), generator=g)])[None]
forced = {3 + 4 * i: seg for i in range(objects)}
seen = {}
_forward = vlm.LlamaDecoder.forward


def forward(self, x):                   # the prefill's row count (the spliced prompt): the first token is emitted by row S - 1
    seen["S"] = self.pos + x.shape[0]
    return _forward(self, x)


vlm.LlamaDecoder.forward = forward


def run(c):
    m = synth.install_forced_tokens(VideoGLaMMForCausalLM(sd, c, torch_dtype=torch.bfloat16, device=dev))
    m.capture = {}
    out_ids, segs = m.inference([images], [context], [sam], ids, [(S, S)], [(src, src)], max_new_tokens=new)
    dec = m.P._decoder
    n = out_ids.shape[1] - ids.shape[1]
    rows = dec.hid_all[seen["S"] - 1:seen["S"] - 1 + n].float()        # the final-norm states that emitted the n tokens
    logits = (rows @ m.P.t("lm_head.weight").float().t()).cpu()
    masks = np.stack([np.stack([segs[0][t][k] for k in sorted(segs[0][t])]) for t in sorted(segs[0])])
    cap = dict(emb=m.capture["emb"].float().cpu(), argmax=list(m.capture["argmax"]))
    del m.P._decoder
    return out_ids[0].tolist(), logits, masks, cap


def report(what, ids4, lg4, got, cap4):
    assert ids4 == ids16
    rel = (lg16 - lg4).norm(dim=1) / lg16.norm(dim=1)
    cos = torch.nn.functional.cosine_similarity(lg16, lg4)
    free = [i for i in range(len(emitted)) if i not in forced]
    agree = sum(cap16["argmax"][i] == cap4["argmax"][i] for i in free) / max(len(free), 1)
    ecos = torch.nn.functional.cosine_similarity(cap16["emb"], cap4["emb"]).min().item()
    iou = np.array([[float((got[t, n] & ref[t, n]).sum() / max((got[t, n] | ref[t, n]).sum(), 1)) for n in range(ref.shape[1])] for t in range(T)])
    print(f"{what} vs bf16 (synthetic weights, {ref.shape[1]} objects x {T} frames, {len(emitted)} steps): logits rel err per step max {rel.max():.3f} "
          f"mean {rel.mean():.3f}, cosine min {cos.min():.4f}, argmax agreement {agree:.2f} of the {len(free)} free steps, [SEG] embedding cosine min {ecos:.4f}, "
          f"mask IoU mean {iou.mean():.4f} min {iou.min():.4f}")
    print("   per-mask [t][n]:", np.round(iou, 3).tolist())


ids16, lg16, ref, cap16 = run(dict(cfg, forced_tokens=forced))
emitted = ids16[ids.shape[1]:]
teacher = {i: t for i, t in enumerate(emitted)}
report("mxfp4 decode weights", *run(dict(cfg, llm=dict(cfg["llm"], decode_weights="mxfp4"), forced_tokens=teacher)))
# the third run: the prompt goes through the 4-bit MLP too (prefill_gemm = "mxfp4": e4m3 activations x the same packed rows; q|k|v and o on vg_gemm_f8)
report("mxfp4 prefill + mxfp4 decode weights", *run(dict(cfg, llm=dict(cfg["llm"], decode_weights="mxfp4", prefill_gemm="mxfp4"), forced_tokens=teacher)))
