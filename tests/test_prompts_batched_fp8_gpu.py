"""The batched multi-prompt decode step with fp8 decode weights (cfg["llm"]["decode_weights"] = "fp8") on the HIP kernels: the B-row
fp8 GEMV gives each row the bits of vg_decode_gemv_w8 on that row alone, and prompts.generate_prompts() on the batched step returns exactly what
its sequential loop (VG_PROMPTS_BATCHED=0) returns, on the Llama-3-8B-width rope step and on the Phi-3-mini-width decode_attention step."""
import functools

import pytest
import torch

import test_prompts_batched_gpu as llama
import test_prompts_batched_phi3_gpu as phi3

torch.set_grad_enabled(False)

ROWS = [1, 2, 3, 5, 8, 16]
PAD = 64            # elements a padded row is longer than the row itself (ldx / ldy / ldr > row length)

# (name, N, K, norm, glu, residual, fp32 out, padded rows)
SHAPES = [
    ("llama gate|up", 14336, 4096, True, True, False, False, False),
    ("llama down", 4096, 14336, False, False, True, False, True),
    ("llama lm_head", 128256, 4096, False, False, False, True, False),
    ("phi3 gate|up", 8192, 3072, True, True, False, False, True),
    ("phi3 down", 3072, 8192, False, False, True, False, False),
    ("phi3 lm_head", 32065, 3072, False, False, False, True, False),
    ("odd N", 1001, 4096, False, False, False, False, True),
]


@functools.lru_cache(maxsize=None)
def _w8(rows, K, seed):
    """fp8 codes + row scales of a random [rows, K] weight (made on the device: the lm_head is 128256 x 4096), and the bf16 weight's device"""
    from videoglamm_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    w = (torch.randn(rows, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16)
    q, sc = ops.quantize_fp8_rows(w)
    return q, sc


def _padded(t, pad):
    """the same values as rows of a wider buffer (row stride = row length + PAD) when pad, else t"""
    if not pad:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + PAD), 7.0, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _inputs(cuda, B, N, K, norm, res, odt, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, K, generator=g) * (2.0 if norm else 0.5)).to(torch.bfloat16).to(cuda)      # every row its own values
    nw = (1.0 + 0.1 * torch.randn(K, generator=g)).to(cuda) if norm else None
    r = torch.randn(B, N, generator=g).to(odt).to(cuda) if res else None
    return x, nw, r


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0].replace(" ", "_") for s in SHAPES])
@pytest.mark.parametrize("B", ROWS)
def test_gemv_w8_rows_bitwise(cuda, B, shape):
    """row r of vg_decode_gemv_w8_rows == vg_decode_gemv_w8 on row r alone, bit for bit, at the shapes of the two models' MLPs and lm_heads"""
    from videoglamm_amd import ops
    _, N, K, norm, glu, res, f32, pad = shape
    odt = torch.float32 if f32 else torch.bfloat16
    q, sc = _w8(2 * N if glu else N, K, N + K)
    x, nw, r = _inputs(cuda, B, N, K, norm, res, odt, 100 * B + 1)
    assert B == 1 or not torch.equal(x[0], x[1])
    xin, rin = _padded(x, pad), None if r is None else _padded(r, pad)
    out = buf = None
    if pad:
        buf = torch.full((B, N + PAD), -3.0, dtype=odt, device=cuda)
        out = buf[:, :N]
        assert xin.stride(0) == K + PAD and out.stride(0) == N + PAD and (rin is None or rin.stride(0) == N + PAD)
    got = ops.decode_gemv_w8_rows(xin, q, sc, norm_w=nw, eps=1e-5, residual=rin, glu=glu, out_dtype=odt, out=out)
    assert got.shape == (B, N) and got.dtype == odt
    for b in range(B):
        want = ops.decode_gemv_w8(x[b:b + 1].contiguous(), q, sc, norm_w=nw, eps=1e-5, residual=None if r is None else r[b:b + 1].contiguous(),
                                  glu=glu, out_dtype=odt)
        assert torch.equal(got[b:b + 1], want), (shape[0], B, b)
    if pad:                                                     # nothing is written between the rows
        assert bool((buf[:, N:] == -3.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,glu,norm,res", [(14336, 4096, True, True, False), (4096, 14336, False, False, True), (3072, 8192, False, False, False),
                                              (9216, 3072, False, True, False)])
def test_gemv_w8_rows_against_the_fp32_statement(cuda, N, K, glu, norm, res):
    """one case per row length against test_decode_gemv_w8's statement (the fp32 product with the dequantised weights, bf16 roundings of the
    norm and of SwiGLU) with that test's tolerances — independent of the single-row kernel"""
    from videoglamm_amd import ops
    B = 5
    q, sc = _w8(2 * N if glu else N, K, 7 + N + K)
    deq = q.view(torch.float8_e4m3fn).float().cpu() * sc.cpu()[:, None]
    x, nw, r = _inputs(cuda, B, N, K, norm, res, torch.bfloat16, 9)
    y = ops.decode_gemv_w8_rows(x, q, sc, norm_w=nw, eps=1e-5, residual=r, glu=glu)
    xf = x.float().cpu()
    if nw is not None:
        xf = ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(torch.bfloat16).float() * nw.cpu()).to(torch.bfloat16).float()
    acc = xf @ deq.t()
    if glu:
        gt, up = acc[:, :N].to(torch.bfloat16).float(), acc[:, N:].to(torch.bfloat16).float()
        acc = torch.nn.functional.silu(gt).to(torch.bfloat16).float() * up
    if r is not None:
        acc = acc + r.float().cpu()
    assert torch.isfinite(y).all() and float(acc.abs().max()) > 0.1
    torch.testing.assert_close(y.float().cpu(), acc.to(torch.bfloat16).float(), rtol=2e-2, atol=2e-2)
    if not glu and r is None:
        yf = ops.decode_gemv_w8_rows(x, q, sc, norm_w=nw, eps=1e-5, out_dtype=torch.float32)
        torch.testing.assert_close(yf.cpu(), acc, rtol=2e-3, atol=2e-3)


@pytest.mark.gpu
def test_refusals_and_supported_query(cuda):
    from videoglamm_amd import _lib, ops
    for K in (3072, 4096, 8192, 14336):
        assert ops.decode_gemv_w8_rows_supported(K)
    q, sc = _w8(256, 8192, 3)
    for K in (1024, 2048, 5120, 6144, 16384):                  # the query agrees with the launcher
        assert not ops.decode_gemv_w8_rows_supported(K)
        if K <= 8192:
            qk = q[:, :K].contiguous()
            with pytest.raises(_lib.VGKernelError):
                ops.decode_gemv_w8_rows(torch.zeros(2, K, dtype=torch.bfloat16, device=cuda), qk, sc)
    ops.decode_gemv_w8_rows(torch.zeros(16, 8192, dtype=torch.bfloat16, device=cuda), q, sc)
    with pytest.raises(_lib.VGKernelError):
        ops.decode_gemv_w8_rows(torch.zeros(17, 8192, dtype=torch.bfloat16, device=cuda), q, sc)
    with pytest.raises(_lib.VGKernelError):
        ops.decode_gemv_w8_rows(torch.zeros(0, 8192, dtype=torch.bfloat16, device=cuda), q, sc)
    with pytest.raises(_lib.VGKernelError):                     # a norm stages whole rows: 16 x 8192 x 2 bytes do not fit
        ops.decode_gemv_w8_rows(torch.zeros(16, 8192, dtype=torch.bfloat16, device=cuda), q, sc, norm_w=torch.ones(8192, device=cuda), eps=1e-5)


# ------------------------------------------------------------------ end to end: the batched route against VG_PROMPTS_BATCHED=0
MODELS = {"llama": llama, "phi3": phi3}
_run, _prompts = llama._run, llama._prompts                     # the two files' helpers are the same code


def _both(monkeypatch, *a, **kw):
    return llama._both(monkeypatch, *a, **kw)


def _llm(cuda, model, prefill=None):
    """the 2-layer synthetic LLM of the bf16 batched tests with fp8 decode weights (and, prefill="fp8", the fp8 prefill GEMMs)"""
    P, cfg, tw = MODELS[model]._llm(cuda)
    c = dict(cfg["llm"], decode_weights="fp8")
    if prefill:
        c["prefill_gemm"] = prefill
    return P, dict(cfg, llm=c), tw


def _rows(P, model):
    rows = next(iter(P._decoder._rows.values()))
    assert P._decoder.w8 and rows.dec is P._decoder and rows.attn_rows == (model == "phi3")
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("B", [2, 5, 16])
def test_greedy_batched_equals_sequential(cuda, monkeypatch, model, B):
    P, cfg, tw = _llm(cuda, model)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None        # a forced [SEG] from the suffix prefill's row and from decode rows
    ref, got = _both(monkeypatch, P, cfg, tw, _prompts(B), 8, hook=hook)
    llama._same(ref, got)
    assert all(len(e) == 2 for e in got[1])
    rows = _rows(P, model)
    assert rows.B == (2 if B == 2 else 8 if B == 5 else 16) and rows.steps == 7


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_fp8_prefill_too(cuda, monkeypatch, model):
    P, cfg, tw = _llm(cuda, model, prefill="fp8")
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step == 2 else None
    ref, got = _both(monkeypatch, P, cfg, tw, _prompts(5, 8), 8, hook=hook)
    llama._same(ref, got)
    assert P._decoder.f8_prefill and _rows(P, model).steps == 7


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_seventeen_prompts_in_groups_of_sixteen(cuda, monkeypatch, model):
    P, cfg, tw = _llm(cuda, model)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None
    ids = _prompts(17, 6)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, ids, 8, hook=hook)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    P._decoder._rows = {}
    a = _run(P, cfg, tw, ids[:16], 8, hook=hook)
    rows = _rows(P, model)
    assert rows.B == 16 and rows.steps == 7
    b = _run(P, cfg, tw, ids[16:], 8, hook=hook)                # one prompt: the single-row fp8 step
    llama._same(ref, (a[0] + b[0], a[1] + b[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_eos_at_different_steps(cuda, monkeypatch, model):
    P, cfg, tw = _llm(cuda, model)
    ids = _prompts(6, 2)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    free, _ = _run(P, cfg, tw, ids, 12)
    eos = sorted({o[len(x) + 1 + b % 6] for b, (o, x) in enumerate(zip(free, ids))})
    ref, got = _both(monkeypatch, P, cfg, tw, ids, 12, eos=eos)
    llama._same(ref, got)
    assert len({len(o) - len(x) for o, x in zip(got[0], ids)}) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("k", [20, 0])          # fast route (1 <= k <= 64) / general route
@pytest.mark.parametrize("B", [2, 5, 16])
def test_sampled_batched_equals_sequential(cuda, monkeypatch, model, B, k):
    P, cfg, tw = _llm(cuda, model)
    sp = [dict(T=0.8, k=k, p=0.9, seed=100 + b) for b in range(B)]
    traces_a, traces_b = [{} for _ in range(B)], [{} for _ in range(B)]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp, traces=traces_a)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp, traces=traces_b)
    llama._same(ref, got)
    assert traces_a == traces_b
    assert _rows(P, model).route == ("sample_fast" if k else "sample")


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_graph_replay_equals_eager(cuda, monkeypatch, model):
    """the captured step against the eager one; the eager step is also counted: per step two fp8 B-row GEMVs per layer and the lm_head, and the
    bf16 B-row GEMV only for the attention projections"""
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, tw = _llm(cuda, model)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step == 3 else None
    ids = _prompts(5, 4)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    a = _run(P, cfg, tw, ids, 8, hook=hook)
    assert _rows(P, model).graphs
    P._decoder = LlamaDecoder(P, cfg["llm"], 1024, use_graph=False)
    calls = {"w8": 0, "bf16": 0}
    w8_rows, bf16_rows = ops.decode_gemv_w8_rows, ops.decode_gemv_rows
    monkeypatch.setattr(ops, "decode_gemv_w8_rows", lambda *x, **kw: (calls.__setitem__("w8", calls["w8"] + 1), w8_rows(*x, **kw))[1])
    monkeypatch.setattr(ops, "decode_gemv_rows", lambda *x, **kw: (calls.__setitem__("bf16", calls["bf16"] + 1), bf16_rows(*x, **kw))[1])
    b = _run(P, cfg, tw, ids, 8, hook=hook)
    rows = _rows(P, model)
    assert not rows.graphs
    llama._same(a, b)
    layers = cfg["llm"]["num_layers"]
    assert calls["w8"] == rows.steps * (2 * layers + 1)
    assert calls["bf16"] == rows.steps * layers * (2 if model == "phi3" else 1)     # q|k|v (decode_attention path) and o


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_batched_route_is_taken(cuda, monkeypatch, model):
    """at B = 8 the batched step runs as many steps as the longest prompt decodes, not their sum (on the sequential loop no RowsDecode exists)"""
    P, cfg, tw = _llm(cuda, model)
    ids = _prompts(8, 5)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    free, _ = _run(P, cfg, tw, ids, 10)
    assert not getattr(P._decoder, "_rows", None)
    eos = [free[0][len(ids[0]) + 3]]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got, _ = _run(P, cfg, tw, ids, 10, eos=eos)
    rows = _rows(P, model)
    gen = [len(o) - len(x) for o, x in zip(got, ids)]
    assert rows.B == 8 and rows.steps == max(gen) - 1 and rows.steps < sum(gen) - len(gen)
