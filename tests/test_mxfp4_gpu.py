"""MXFP4 decode weights (cfg["llm"]["decode_weights"] = "mxfp4") on the HIP kernels: vg_decode_gemv_w4 against the fp32 product with the
dequantised weights, the decode step against its exact bf16 twin (the bf16 decode path on the dequantised MLP weights), graph replay against the
eager step, and the façade (inference_prompts() entry b == inference() on prompt b)."""
import numpy as np
import pytest
import torch

from test_e2e_fp8_gpu import _cfg
from test_host_vlm import ops_decode_row

torch.set_grad_enabled(False)


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["packed", "separate"])
@pytest.mark.parametrize("N,K,glu,norm,res", [(4096, 4096, False, False, True), (6144, 4096, False, True, False), (14336, 4096, True, True, False),
                                              (4096, 14336, False, False, True), (3072, 8192, False, False, False), (9216, 3072, False, True, False),
                                              (8192, 3072, True, True, False), (1001, 4096, False, False, False)])
def test_decode_gemv_w4(cuda, N, K, glu, norm, res, layout):
    """test_decode_gemv_w8's cases and tolerances (the only difference to that kernel is the weight format): the fp32 product with the DEQUANTISED
    weights, bf16 out rtol = atol = 2e-2, fp32 out 2e-3; both weight layouts; an unsupported row length raises."""
    from videoglamm_amd import _lib, ops
    rows = 2 * N if glu else N
    w = rnd(rows, K, seed=1, scale=K ** -0.5)
    x = rnd(1, K, dtype=torch.bfloat16, seed=2)
    nw = (1.0 + 0.1 * rnd(K, seed=3)) if norm else None
    r = rnd(1, N, dtype=torch.bfloat16, seed=4) if res else None
    codes, scales = ops.quantize_mxfp4_rows(w.to(cuda))
    deq = ops.mxfp4_dequant(codes, scales).cpu()
    amax = w.reshape(rows, K // 32, 32).abs().amax(dim=-1, keepdim=True)
    assert bool(((deq - w).reshape(rows, K // 32, 32).abs() <= 0.25 * amax).all())
    wargs = (ops.mxfp4_pack(codes, scales),) if layout == "packed" else (codes, scales)
    kw = dict(norm_w=None if nw is None else nw.to(cuda), eps=1e-5, glu=glu)
    y = ops.decode_gemv_w4(x.to(cuda), *wargs, residual=None if r is None else r.to(cuda), **kw)
    xf = x.float()
    if nw is not None:
        xf = ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(torch.bfloat16).float() * nw).to(torch.bfloat16).float()
    acc = xf @ deq.t()
    if glu:
        g, u = acc[:, :N].to(torch.bfloat16).float(), acc[:, N:].to(torch.bfloat16).float()
        acc = torch.nn.functional.silu(g).to(torch.bfloat16).float() * u
    if r is not None:
        acc = acc + r.float()
    assert y.dtype == torch.bfloat16 and y.shape == (1, N)
    err = (y.float().cpu() - acc.to(torch.bfloat16).float()).abs()
    print(f"w4 {layout} N={N} K={K} glu={glu} norm={norm} res={res}: bf16 out max abs err {err.max():.3e}")
    torch.testing.assert_close(y.float().cpu(), acc.to(torch.bfloat16).float(), rtol=2e-2, atol=2e-2)
    yf = ops.decode_gemv_w4(x.to(cuda), *wargs, out_dtype=torch.float32, **kw)
    assert yf.dtype == torch.float32
    if not glu and r is None:
        print(f"   fp32 out max abs err {(yf.cpu() - acc).abs().max():.3e}")
        torch.testing.assert_close(yf.cpu(), acc, rtol=2e-3, atol=2e-3)
    with pytest.raises(_lib.VGKernelError):
        ops.decode_gemv_w4(x.to(cuda)[:, :1024].contiguous(), codes[:, :512].contiguous(), scales[:, :32].contiguous())
    with pytest.raises(_lib.VGKernelError):
        ops.decode_gemv_w4(x.to(cuda)[:, :2048].contiguous(), wargs[0])


def _decoder_sd(cuda, c):
    from videoglamm_amd import synth
    base = synth.videoglamm_phi3_mini() if c["hidden"] == 3072 else synth.videoglamm_llama3_8b()
    man = {k: v for k, v in synth.vlm_manifest(dict(base, llm=c)).items()
           if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))}
    return synth.device_state_dict(man, cuda, torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("width", ["llama3-8b", "phi3-mini"])
def test_decode_step_equals_its_bf16_twin(cuda, width):
    """Run A: decode_weights = "mxfp4".  Run B: the bf16 decode path on a state dict whose MLP weights were replaced by their dequantised MXFP4
    values (exact in bf16).  Both compute the same products; they differ in summation order and in the bf16 roundings a reordered sum can flip.
    Compared: the final-norm rows of seven steps (relative error < 1e-2 per row), and — logits formed here from both sets of rows and ONE lm_head
    matrix — the argmax wherever B's top-2 margin exceeds four times the rms difference of the two logit rows."""
    from videoglamm_amd import ops, synth
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    c = dict(synth.PHI3_MINI if width == "phi3-mini" else synth.LLAMA3_8B, num_layers=2, vocab=4096)
    sd = _decoder_sd(cuda, c)
    twin = dict(sd)
    nmlp = 0
    for k, v in sd.items():
        if ".mlp." in k and k.endswith(".weight"):
            deq = ops.mxfp4_dequant(*ops.quantize_mxfp4_rows(v))
            twin[k] = deq.to(torch.bfloat16)
            assert torch.equal(twin[k].float(), deq)
            nmlp += 1
    assert nmlp == 2 * (2 if width == "phi3-mini" else 3)
    x = (torch.randn(46, c["hidden"], generator=torch.Generator().manual_seed(3)) * 0.5).to(cuda, torch.bfloat16)
    # both runs prefill (bf16 GEMMs) on the twin's weights, so they start the decode steps from the same KV cache; run A's MXFP4 copies are those of
    # the original checkpoint: the dequantised weights are a fixed point of the quantiser
    decs = []
    for mode in ("mxfp4", "bf16"):
        dec = LlamaDecoder(Params(twin, cuda, torch.bfloat16), dict(c, decode_weights=mode), 1024, use_graph=False)
        assert dec.w4 == (mode == "mxfp4") and not dec.w8 and dec.fused_decode
        dec.forward(x[:39])
        decs.append(dec)
    a, b = decs
    l0 = "model.layers.0.mlp."
    assert torch.equal(ops.mxfp4_dequant(a.P.fp4(l0 + "down_proj")), ops.mxfp4_dequant(Params(sd, cuda, torch.bfloat16).fp4(l0 + "down_proj")))
    assert torch.equal(ops.mxfp4_dequant(a.P.fp4(l0 + "down_proj")).to(torch.bfloat16), b.P.w(l0 + "down_proj"))
    rows = []
    for dec in (a, b):
        rows.append(torch.cat([ops_decode_row(dec, x[39 + i:40 + i]) for i in range(7)]).float().cpu())
    ha, hb = rows
    rel = ((ha - hb).norm(dim=1) / hb.norm(dim=1))
    lm = sd["lm_head.weight"].float().cpu()
    la, lb = ha @ lm.t(), hb @ lm.t()
    top2 = lb.topk(2, dim=1).values
    margin, noise = top2[:, 0] - top2[:, 1], (la - lb).pow(2).mean(dim=1).sqrt()
    clear = margin > 4 * noise
    agree = la.argmax(1) == lb.argmax(1)
    print(f"mxfp4 decode step vs its bf16 twin ({width}): relative error per row max {rel.max():.3e} (rows {[f'{v:.2e}' for v in rel.tolist()]}), "
          f"clear-margin steps {int(clear.sum())}/7, argmax agreement {int(agree.sum())}/7")
    assert float(rel.max()) < 1e-2, rel.tolist()
    assert bool(agree[clear].all()), "an argmax with a clear margin differs between the mxfp4 step and its bf16 twin"
    # and the lm_head of the mxfp4 decoder is the fp8 GEMV
    calls = []
    w8 = ops.decode_gemv_w8
    try:
        ops.decode_gemv_w8 = lambda *p, **kw: (calls.append(1), w8(*p, **kw))[1]
        a.next_token(torch.cat([ops_decode_row(a, x[45:46])]))
    finally:
        ops.decode_gemv_w8 = w8
    assert len(calls) == 1


@pytest.mark.gpu
def test_graph_replay_equals_eager(cuda):
    """the captured decode step with "mxfp4" emits the ids of the eager step: 32 decoded tokens after the prefill's on the 2-layer decoder of
    Llama-3-8B width; the eager step is counted too: two MXFP4 GEMVs per layer for every fp8 GEMV (the lm_head)"""
    from videoglamm_amd import ops, synth
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder, decode_loop
    c = dict(synth.LLAMA3_8B, num_layers=2, vocab=4096, decode_weights="mxfp4")
    P = Params(_decoder_sd(cuda, c), cuda, torch.bfloat16)
    x = (torch.randn(40, c["hidden"], generator=torch.Generator().manual_seed(5)) * 0.5).to(cuda, torch.bfloat16)
    ids = []
    calls = {"w4": 0, "w8": 0}
    w4, w8 = ops.decode_gemv_w4, ops.decode_gemv_w8
    for graph in (True, False):
        dec = LlamaDecoder(P, c, 1024, use_graph=graph)
        dec.next_token(dec.forward(x)[-1:])
        toks = []
        try:
            if not graph:
                ops.decode_gemv_w4 = lambda *p, **kw: (calls.__setitem__("w4", calls["w4"] + 1), w4(*p, **kw))[1]
                ops.decode_gemv_w8 = lambda *p, **kw: (calls.__setitem__("w8", calls["w8"] + 1), w8(*p, **kw))[1]
            decode_loop(P, dec, toks, 33, set())
        finally:
            ops.decode_gemv_w4, ops.decode_gemv_w8 = w4, w8
        assert bool(dec.graphs) == graph
        ids.append(toks)
    print("mxfp4 graph replay vs eager ids:", ids[0][:8], "...")
    assert ids[0] == ids[1] and len(ids[0]) == 33
    assert calls["w8"] >= 32 and calls["w4"] == 2 * c["num_layers"] * calls["w8"]


def _facade(cuda, video, monkeypatch):
    """inference() per prompt and one 3-prompt inference_prompts() on the micro model of test_e2e_fp8_gpu.py with decode_weights = "mxfp4", two
    forced [SEG] objects per prompt -> (inference() results, inference_prompts() results, the model)"""
    from videoglamm_amd import synth
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    cfg = _cfg()
    cfg["llm"] = dict(cfg["llm"], decode_weights="mxfp4")
    te, T, hw = 4, 3, (48, 64)
    sd = synth.device_state_dict(synth.manifest(cfg), cuda, torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    images, context = torch.randn(te, 3, 224, 224, generator=g).to(cuda), torch.randn(te, 3, 336, 336, generator=g).to(cuda)
    sam = torch.randn(T, 3, 256, 256, generator=g).to(cuda)
    head = torch.cat([torch.tensor([1, 5, 6]), torch.full((te,), -200)])
    ids = [torch.cat([head, torch.randint(3, 4000, (n,), generator=g)]) for n in (20, 7, 13)]
    m = VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.bfloat16, device=cuda)
    seg = cfg["seg_token_idx"]
    m.token_hook = lambda step, tok: seg if step in (2, 5) else None
    clip, rest = ([images], [context], [sam]), ([(256, 256)], [hw])
    ref = [m.inference(*clip, x[None], *rest, max_new_tokens=10, use_sam2_video_branch=video) for x in ids]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got = m.inference_prompts(*clip, ids, *rest, max_new_tokens=10, use_sam2_video_branch=video)
    return ref, got, m


def _stack(segs):
    return np.stack([np.stack([segs[t][k] for k in sorted(segs[t])]) for t in sorted(segs)])


@pytest.mark.gpu
@pytest.mark.parametrize("video", [False, True])
def test_facade_prompts_ids_equal_inference(cuda, video, monkeypatch):
    """inference_prompts() entry b emits the ids inference() emits on prompt b, with the same objects per frame — a batched route that decoded an
    "mxfp4" model on bf16 weights would not; the decoder behind both calls is the mxfp4 one and no batched state is built (there is no B-row
    MXFP4 GEMV).  A prompt without a [SEG] gets {} on both branches."""
    ref, (out, segs), m = _facade(cuda, video, monkeypatch)
    dec = m.P._decoder
    assert dec.w4 and not dec.w8 and not getattr(dec, "_rows", None)
    for b, (o, s) in enumerate(ref):
        assert torch.equal(out[b].reshape(-1), o.reshape(-1)), b
        assert sorted(segs[b]) == sorted(s[0]) and len(s[0]) > 0 and all(sorted(segs[b][t]) == sorted(s[0][t]) for t in s[0])
    m.token_hook = None                      # random weights never emit [SEG]
    m.capture = {}
    g = torch.Generator().manual_seed(5)
    te = 4
    images, context = torch.randn(te, 3, 224, 224, generator=g).to(cuda), torch.randn(te, 3, 336, 336, generator=g).to(cuda)
    sam = torch.randn(3, 3, 256, 256, generator=g).to(cuda)
    head = torch.cat([torch.tensor([1, 5, 6]), torch.full((te,), -200)])
    ids = [torch.cat([head, torch.tensor([9, 8, 7])]), torch.cat([head, torch.tensor([11, 12])])]
    out, segs = m.inference_prompts([images], [context], [sam], ids, [(256, 256)], [(48, 64)], max_new_tokens=4, use_sam2_video_branch=video)
    assert segs == [{}, {}] and [o.shape for o in out] == [(1, len(x) + 4) for x in ids]
    assert len(m.capture["argmax"]) == 2 and all(len(a) == 4 for a in m.capture["argmax"]) and all(e.shape[0] == 0 for e in m.capture["emb"])


@pytest.mark.gpu
@pytest.mark.parametrize("video", [False, True])
def test_facade_prompts_masks_equal_inference(cuda, video, monkeypatch):
    """inference_prompts() entry b gives the masks inference() gives on prompt b, pixel for pixel, on both SAM2 branches.  In bf16 that holds only
    when entry b is computed by the calls inference() makes: the shared route of the other modes (one SAM2 call with every prompt's objects, suffix
    prefills on top of the shared prefix) differs from inference() by 26 - 62 of 18432 pixels per prompt on this micro model (measured, MI355X,
    decode_weights None / "fp8", and "mxfp4" when it was sent down that route) — so an "mxfp4" model, which has no batched step to gain from, runs
    its prompts as inference() does."""
    ref, (out, segs), m = _facade(cuda, video, monkeypatch)
    worst = []
    for b, (o, s) in enumerate(ref):
        m_got, m_ref = _stack(segs[b]), _stack(s[0])
        iou = (m_got & m_ref).sum() / max((m_got | m_ref).sum(), 1)
        print(f"mxfp4 facade ({'video' if video else 'framewise'} branch) prompt {b}: {m_ref.shape[1]} objects x {m_ref.shape[0]} frames, "
              f"mask IoU vs inference() {iou:.6f}, differing pixels {int((m_got != m_ref).sum())} of {m_ref.size}")
        worst.append((b, float(iou), int((m_got != m_ref).sum())))
    assert all(n == 0 for _, _, n in worst), worst
