"""cfg["llm"]["prefill_gemm"] = "mxfp4" and cfg["llm"]["dense_mlp"] = "drop" on the HIP kernels: 2-layer decoders of Llama-3-8B and Phi-3-mini width
(vocab 4096, 300 prompt rows, as test_prefill_fp8_hip builds them), and the micro façade model of the mxfp4 decode tests."""
import gc

import numpy as np
import pytest
import torch

from test_host_vlm import ops_decode_row
from test_prompts_batched_mxfp4_gpu import _micro

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BF = torch.bfloat16


def _llm(cuda, model):
    """(llm cfg, device state dict of the LLM alone, 300 embedding rows)"""
    from videoglamm_amd import synth
    full = synth.videoglamm_llama3_8b() if model == "llama" else synth.videoglamm_phi3_mini()
    c = dict(full["llm"], num_layers=2, vocab=4096)
    man = {k: v for k, v in synth.vlm_manifest(dict(full, llm=c)).items()
           if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))}
    sd = synth.device_state_dict(man, cuda, BF)
    x = (torch.randn(300, c["hidden"], generator=torch.Generator().manual_seed(4)) * 0.5).to(cuda, BF)
    return c, sd, x


def _mlp_names(P, c):
    for i in range(c["num_layers"]):
        l = f"model.layers.{i}."
        yield l, [l + "mlp.gate_proj", l + "mlp.up_proj"], l + "mlp.gate_up_proj", l + "mlp.down_proj"


@pytest.mark.parametrize("model", ["llama", "phi3"])
def test_mode_against_its_bf16_twin(cuda, model):
    """prefill_gemm = "mxfp4" against the bf16 prefill of the SAME weights: a state dict whose MLP weights are ops.mxfp4_dequant of the packed rows
    (exact in bf16).  What separates the two is e4m3 activations on four GEMMs and e4m3 attention-projection weights — a subset of what separates
    "fp8" from bf16 — so test_prefill_fp8_hip's bound holds: min cosine > 0.995, max relative row error < 0.10.  Row 300 is a decode step on the
    K/V cache each mode left.  Measured on an MI355X (min cosine, max relative row error; the decode row alone): Llama-3-8B width 0.99606, 0.0887
    (0.0216); Phi-3-mini width 0.99631, 0.0859 (0.0228) — also in DESIGN.md section 8."""
    from videoglamm_amd import ops
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    c, sd, x = _llm(cuda, model)
    P4 = Params(sd, cuda, BF)
    twin = dict(sd)
    for l, gu, stored, down in _mlp_names(P4, c):
        wgu = ops.mxfp4_dequant(P4.fp4(gu, stored=stored)).to(BF)
        assert torch.equal(wgu.float(), ops.mxfp4_dequant(P4.fp4(gu, stored=stored)))          # exact in bf16
        if stored + ".weight" in sd:
            twin[stored + ".weight"] = wgu
        else:
            twin[gu[0] + ".weight"], twin[gu[1] + ".weight"] = wgu[: c["ffn"]].contiguous(), wgu[c["ffn"]:].contiguous()
        twin[down + ".weight"] = ops.mxfp4_dequant(P4.fp4(down)).to(BF)
    hs = []
    # (the mode's decoder decodes on the packed rows too, decode_weights = "mxfp4": its step then multiplies by the twin's weights exactly)
    for P, cm in ((Params(twin, cuda, BF), dict(c, prefill_gemm="bf16")), (P4, dict(c, prefill_gemm="mxfp4", decode_weights="mxfp4"))):
        dec = LlamaDecoder(P, cm, 1024, use_graph=False)
        h = dec.forward(x[:299])
        hs.append(torch.cat([h, ops_decode_row(dec, x[299:300])]).float().cpu())
    cos = torch.nn.functional.cosine_similarity(hs[0], hs[1]).min().item()
    rel = ((hs[0] - hs[1]).norm(dim=1) / hs[0].norm(dim=1)).max().item()
    rel_step = ((hs[0][299] - hs[1][299]).norm() / hs[0][299].norm()).item()
    print(f"prefill mxfp4 vs its bf16 twin ({model}): min cosine {cos:.5f}, max relative row error {rel:.4f} (the decode step, row 300: {rel_step:.4f})")
    assert cos > 0.995 and rel < 0.10, (cos, rel)


@pytest.mark.parametrize("model", ["llama", "phi3"])
def test_short_prefill_takes_the_rows_gemv(cuda, model):
    """a 12-row prefill runs its MLP on ops.decode_gemv_w4_rows: one layer rebuilt from the ops calls equals the decoder's bit for bit"""
    from videoglamm_amd import ops
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    c, sd, x = _llm(cuda, model)
    c1 = dict(c, num_layers=1, prefill_gemm="mxfp4")
    P = Params(sd, cuda, BF)
    dec = LlamaDecoder(P, c1, 1024, use_graph=False)
    got = dec.forward(x[:12])
    # the expectation: layer 0 from the ops calls
    l = "model.layers.0."
    H, Hkv, hd = dec.H, dec.Hkv, dec.hd
    x0 = x[:12]
    h = ops.rmsnorm(x0, P.f32(l + "input_layernorm.weight"), c["rms_eps"])
    wqkv, _ = P.fused([l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj"], stored=l + "self_attn.qkv_proj")
    qkv = ops.linear(h, wqkv)
    kc, vc = torch.zeros_like(dec.kc[0]), torch.zeros_like(dec.vc[0])
    ops.rope_kv_append_(qkv, kc, vc, dec.cos, dec.sin, H, Hkv, hd, 0, None)
    o = ops.attention(qkv[:, : H * hd].view(1, 12, H, hd), kc[:12].unsqueeze(0), vc[:12].unsqueeze(0), hd ** -0.5, causal=True, window=dec.window)
    x1 = ops.linear(o.view(12, dec.D), P.w(l + "self_attn.o_proj"), residual=x0)
    h = ops.rmsnorm(x1, P.f32(l + "post_attention_layernorm.weight"), c["rms_eps"])
    a = ops.decode_gemv_w4_rows(h, P.fp4([l + "mlp.gate_proj", l + "mlp.up_proj"], stored=l + "mlp.gate_up_proj"), glu=True)
    x2 = ops.decode_gemv_w4_rows(a, P.fp4(l + "mlp.down_proj"), residual=x1)
    want = ops.rmsnorm(x2, P.f32("model.norm.weight"), c["rms_eps"])
    assert torch.equal(got, want)
    # and 20 rows take the tile path, 16 + 4 rows at a device-side position would not: the two routes differ in their arithmetic
    dec.reset()
    assert not torch.equal(dec.forward(x[:20])[:12], want)


@pytest.mark.parametrize("model", ["llama", "phi3"])
def test_dense_mlp_drop(cuda, model):
    """dense_mlp = "drop" changes no number (300-row prefill, 12-row prefill, three decode steps: final-norm rows bit-identical), frees at least the
    bf16 bytes of the two layers' MLP weights, and a dense access then raises"""
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    c, sd, x = _llm(cuda, model)
    c4 = dict(c, prefill_gemm="mxfp4", decode_weights="mxfp4")
    mlp_bytes = 2 * 3 * c["hidden"] * c["ffn"] * c["num_layers"]

    def run(dec):
        out = [dec.forward(x).clone()]                  # the 300-row prefill, then three decode steps on its cache
        out += [ops_decode_row(dec, x[7 * i:7 * i + 1]).clone() for i in range(3)]
        dec.reset()
        out.append(dec.forward(x[:12]).clone())
        return out

    def built(flag):
        """a decoder on a private copy of the state dict that this test holds no reference to, and memory_allocated right after its construction.
        memory_allocated counts whole allocator blocks, so the two builds make the SAME allocations from an allocator that holds no cached block:
        without the flag the packed rows of every layer are built here, as the flag's constructor builds them — what then separates the two
        figures is what Params.drop freed."""
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        own = {k: v.clone() for k, v in sd.items()}
        P = Params(own, cuda, BF)
        del own
        dec = LlamaDecoder(P, dict(c4, dense_mlp=flag), 1024, use_graph=False)
        if flag == "keep":
            for l, gu, stored, down in _mlp_names(P, c):
                P.fp4(gu, stored=stored)
                P.fp4(down)
        torch.cuda.synchronize()
        return dec, torch.cuda.memory_allocated()

    gc.collect()
    base = torch.cuda.memory_allocated()
    dk, mk = built("keep")
    keep = [t.cpu() for t in run(dk)]
    del dk
    dd, md = built("drop")
    print(f"dense_mlp ({model}): allocated with the dense MLP {(mk - base) / 2**20:.1f} MiB, dropped {(md - base) / 2**20:.1f} MiB, "
          f"bf16 MLP bytes {mlp_bytes / 2**20:.1f} MiB")
    assert mk - md >= mlp_bytes, (mk - md, mlp_bytes)
    drop = [t.cpu() for t in run(dd)]
    for a, b in zip(keep, drop):
        assert torch.equal(a, b)
    P = dd.P
    with pytest.raises(KeyError, match="dropped"):
        P.w("model.layers.0.mlp.down_proj")
    with pytest.raises(KeyError, match="dropped"):
        P.fused(["model.layers.1.mlp.gate_proj", "model.layers.1.mlp.up_proj"], stored="model.layers.1.mlp.gate_up_proj")
    assert P.w("model.layers.0.self_attn.o_proj").shape == (c["hidden"], c["hidden"])
    with pytest.raises(RuntimeError, match="dropped"):                      # the same Params under a cfg that needs the dense weights
        LlamaDecoder(P, dict(c, prefill_gemm="bf16"), 1024, use_graph=False)


def test_facade(cuda, monkeypatch):
    """inference() under prefill mxfp4 + decode mxfp4 + drop returns ids and masks; inference_clips on two clips equals inference per clip bit for bit;
    inference_prompts(shared=True) runs; a cast after the drop is refused"""
    m, clip, ids, rest = _micro(cuda, "mxfp4")
    m.cfg["llm"] = dict(m.cfg["llm"], prefill_gemm="mxfp4", dense_mlp="drop")
    kw = dict(max_new_tokens=10, use_sam2_video_branch=False)
    ref = [m.inference(*clip, x[None], *rest, **kw) for x in ids[:2]]
    dec = m.P._decoder
    assert dec.w4_prefill and dec.w4 and dec.dense_dropped and m.P.dropped
    for x, (out, segs) in zip(ids, ref):
        assert out.numel() > 0 and len(segs[0]) > 0
        assert all(isinstance(v, np.ndarray) for t in segs[0] for v in segs[0][t].values())
    clips = [(*clip, x[None], *rest) for x in ids[:2]]
    got = m.inference_clips(clips, **kw)
    for (o, s), (o2, s2) in zip(got, ref):
        assert torch.equal(o, o2) and sorted(s[0]) == sorted(s2[0])
        assert all(np.array_equal(s[0][t][k], s2[0][t][k]) for t in s2[0] for k in s2[0][t])
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    out, segs = m.inference_prompts(*clip, ids, *rest, shared=True, **kw)
    assert len(out) == len(ids) and all(len(s) > 0 for s in segs)
    with pytest.raises(RuntimeError, match="dropped"):
        m.float()
    m.cfg["llm"] = dict(m.cfg["llm"], prefill_gemm="bf16")                  # the live cfg back on a dense mode: refused, not ignored
    with pytest.raises(RuntimeError, match="dropped"):
        m.inference(*clip, ids[0][None], *rest, **kw)
