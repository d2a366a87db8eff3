"""The batched multi-prompt decode step with MXFP4 decode weights (cfg["llm"]["decode_weights"] = "mxfp4") on the HIP kernels: the
B-row MXFP4 GEMV gives each row the bits of vg_decode_gemv_w4 on that row alone (and the exact integers of test_contraction_exact_gpu.py),
prompts.generate_prompts() on the batched step returns exactly what its sequential loop (VG_PROMPTS_BATCHED=0) returns at Llama-3-8B and at
Phi-3-mini width, and inference_prompts(shared=...) picks the route."""
import functools

import numpy as np
import pytest
import torch

import _exact as E
import test_prompts_batched_fp8_gpu as fp8
import test_prompts_batched_gpu as llama
from test_contraction_exact_gpu import _gemv_variants, _rows_norm_fits, _rows_norm_refused
from test_e2e_fp8_gpu import _cfg
from test_mxfp4_gpu import _stack

torch.set_grad_enabled(False)

BF = torch.bfloat16
ROWS = [1, 2, 3, 5, 8, 16]
PAD = 64            # elements a padded row is longer than the row itself (ldx / ldy / ldr > row length)

# (name, K, norm, glu, residual, fp32 out, padded rows, N values).  N = 33: fewer pairs than a workgroup's waves; 1001: an unpaired last row; 4100
# with glu: more than one pair per wave and a ragged last wave; K = 14336 at B >= 8 (and every K at 16 rows without a norm): the phased staging
SHAPES = [
    ("K4096 norm glu", 4096, True, True, False, False, False, (33, 4100)),
    ("K14336 residual padded", 14336, False, False, True, False, True, (33, 1001)),
    ("K3072 norm glu padded", 3072, True, True, False, False, True, (33, 4100)),
    ("K8192 residual", 8192, False, False, True, False, False, (1001,)),
    ("K8192 fp32 out", 8192, False, False, False, True, False, (1001,)),
    ("K4096 plain padded", 4096, False, False, False, False, True, (1001,)),
]
CASES = [(s[0] + f" N{N}", N) + s[1:7] for s in SHAPES for N in s[7]]


@functools.lru_cache(maxsize=None)
def _w4(rows, K, seed):
    """packed MXFP4 rows of a random [rows, K] weight, and the float32 matrix they mean (both on the device)"""
    from videoglamm_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    w = torch.randn(rows, K, generator=g, device=dev) * K ** -0.5
    codes, scales = ops.quantize_mxfp4_rows(w)
    return ops.mxfp4_pack(codes, scales), ops.mxfp4_dequant(codes, scales)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
@pytest.mark.parametrize("B", ROWS)
def test_gemv_w4_rows_bitwise(cuda, B, case):
    """row r of vg_decode_gemv_w4_rows == vg_decode_gemv_w4 on row r alone, bit for bit; padded outputs keep their fill between the rows"""
    from videoglamm_amd import ops
    name, N, K, norm, glu, res, f32, pad = case
    odt = torch.float32 if f32 else BF
    w4, _ = _w4(2 * N if glu else N, K, N + K)
    x, nw, r = fp8._inputs(cuda, B, N, K, norm, res, odt, 100 * B + 1)
    assert B == 1 or not torch.equal(x[0], x[1])
    xin, rin = fp8._padded(x, pad), None if r is None else fp8._padded(r, pad)
    out = buf = None
    if pad:
        buf = torch.full((B, N + PAD), -3.0, dtype=odt, device=cuda)
        out = buf[:, :N]
        assert xin.stride(0) == K + PAD and out.stride(0) == N + PAD and (rin is None or rin.stride(0) == N + PAD)
    got = ops.decode_gemv_w4_rows(xin, w4, norm_w=nw, eps=1e-5, residual=rin, glu=glu, out_dtype=odt, out=out)
    assert got.shape == (B, N) and got.dtype == odt
    for b in range(B):
        want = ops.decode_gemv_w4(x[b:b + 1].contiguous(), w4, norm_w=nw, eps=1e-5, residual=None if r is None else r[b:b + 1].contiguous(),
                                  glu=glu, out_dtype=odt)
        assert torch.equal(got[b:b + 1], want), (name, B, b)
    if pad:                                                     # nothing is written between the rows
        assert bool((buf[:, N:] == -3.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("B", E.W8_ROWS_B)
@pytest.mark.parametrize("K", E.GEMV_Q_K)
def test_decode_gemv_w4_rows_exact(cuda, B, K):
    """the B-row twin of test_contraction_exact_gpu.py::test_decode_gemv_w4 (packed rows inside a 0x77-filled strided buffer with guard rows): every
    variant equals the float64 product bit for bit; where the bucket's rows do not fit the norm's staging the launcher refuses the fused norm"""
    from videoglamm_amd import ops
    assert ops.decode_gemv_w4_rows_supported(K)
    fits = _rows_norm_fits(B, K)
    x, xn, nw = E.ints((B, K), seed=K + B), E.ints((B, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in E.GEMV_Q_N:
        codes, scales, deq, _ = E.mxfp4_rows(2 * N, K, seed=N + K)
        rows_ = ops.mxfp4_pack(codes, scales)
        big = torch.full((2 * N + 2, rows_.shape[1] + 16), 0x77, dtype=torch.uint8)          # gap bytes and guard rows: two +6 codes each
        big[:2 * N, :rows_.shape[1]] = rows_
        strided = big.to(cuda)[:2 * N, :rows_.shape[1]]
        wd = rows_.to(cuda)
        _gemv_variants(cuda, ops.decode_gemv_w4_rows, BF, x, xn, nw, deq, (wd,), (strided,), N, f"decode_gemv_w4_rows B={B} N={N} K={K}", norm=fits)
        if not fits:
            _rows_norm_refused(cuda, ops.decode_gemv_w4_rows, B, K, wd[:N])


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,glu,norm,res", [(4100, 4096, True, True, False), (1001, 14336, False, False, True), (1001, 8192, False, False, False),
                                              (1001, 3072, False, True, False)])
def test_gemv_w4_rows_against_the_fp32_statement(cuda, N, K, glu, norm, res):
    """one case per row length against test_mxfp4_gpu.py::test_decode_gemv_w4's statement (the fp32 product with the dequantised weights, bf16
    roundings of the norm and of SwiGLU) with that test's tolerances (bf16 out rtol = atol = 2e-2, fp32 out 2e-3) — independent of the single-row
    kernel"""
    from videoglamm_amd import ops
    B = 5
    w4, deq = _w4(2 * N if glu else N, K, 7 + N + K)
    deq = deq.cpu()
    x, nw, r = fp8._inputs(cuda, B, N, K, norm, res, BF, 9)
    y = ops.decode_gemv_w4_rows(x, w4, norm_w=nw, eps=1e-5, residual=r, glu=glu)
    xf = x.float().cpu()
    if nw is not None:
        xf = ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(BF).float() * nw.cpu()).to(BF).float()
    acc = xf @ deq.t()
    if glu:
        gt, up = acc[:, :N].to(BF).float(), acc[:, N:].to(BF).float()
        acc = torch.nn.functional.silu(gt).to(BF).float() * up
    if r is not None:
        acc = acc + r.float().cpu()
    assert y.shape == (B, N) and y.dtype == BF and torch.isfinite(y).all() and float(acc.abs().max()) > 0.1
    print(f"w4 rows N={N} K={K} glu={glu} norm={norm} res={res}: bf16 out max abs err {(y.float().cpu() - acc.to(BF).float()).abs().max():.3e}")
    torch.testing.assert_close(y.float().cpu(), acc.to(BF).float(), rtol=2e-2, atol=2e-2)
    if not glu and r is None:
        yf = ops.decode_gemv_w4_rows(x, w4, norm_w=nw, eps=1e-5, out_dtype=torch.float32)
        print(f"   fp32 out max abs err {(yf.cpu() - acc).abs().max():.3e}")
        torch.testing.assert_close(yf.cpu(), acc, rtol=2e-3, atol=2e-3)


@pytest.mark.gpu
def test_refusals_and_supported_query(cuda):
    from videoglamm_amd import _lib, ops
    for K in (3072, 4096, 8192, 14336):
        assert ops.decode_gemv_w4_rows_supported(K)
    w4, _ = _w4(256, 8192, 3)
    zeros = lambda B, K: torch.zeros(B, K, dtype=BF, device=cuda)      # noqa: E731
    for K in (1024, 2048, 5120, 6144, 16384):                  # the query agrees with the launcher
        assert not ops.decode_gemv_w4_rows_supported(K)
        with pytest.raises(_lib.VGKernelError):
            ops.decode_gemv_w4_rows(zeros(2, K), torch.zeros(256, 128 + K // 2, dtype=torch.uint8, device=cuda))
    y = ops.decode_gemv_w4_rows(zeros(16, 8192), w4)           # 16 x 8192 without a norm runs (in phases)
    assert y.shape == (16, 256) and not bool(y.any())
    with pytest.raises(_lib.VGKernelError):
        ops.decode_gemv_w4_rows(zeros(17, 8192), w4)
    with pytest.raises(_lib.VGKernelError):
        ops.decode_gemv_w4_rows(zeros(0, 8192), w4)
    with pytest.raises(_lib.VGKernelError):                     # a norm stages whole rows: 16 x 8192 x 2 bytes do not fit
        ops.decode_gemv_w4_rows(zeros(16, 8192), w4, norm_w=torch.ones(8192, device=cuda), eps=1e-5)
    with pytest.raises(AssertionError):                         # packed rows of another row length (K = 4096's against x of 8192)
        ops.decode_gemv_w4_rows(zeros(2, 8192), _w4(64, 4096, 3)[0])
    with pytest.raises(_lib.VGKernelError):                     # and the launcher's own check: a row stride that does not cover a packed row
        lib = _lib.load()
        xx, yy = zeros(2, 8192), zeros(2, 256)
        _lib.check(lib.vg_decode_gemv_w4_rows(ops._p(xx), 8192, ops._p(w4), 4096, ops._p(yy), 256, None, 0.0, None, 0, 256, 8192, 2, 0, ops.BF16,
                                              ops._stream()), "vg_decode_gemv_w4_rows")


# ------------------------------------------------------------------ end to end: the batched route against VG_PROMPTS_BATCHED=0
MODELS = fp8.MODELS
_run, _prompts, _same = llama._run, llama._prompts, llama._same


def _both(monkeypatch, *a, **kw):
    return llama._both(monkeypatch, *a, **kw)


def _llm(cuda, model):
    """the 2-layer synthetic LLM of the bf16 batched tests with MXFP4 decode weights"""
    P, cfg, tw = MODELS[model]._llm(cuda)
    return P, dict(cfg, llm=dict(cfg["llm"], decode_weights="mxfp4")), tw


def _rows(P, model):
    rows = next(iter(P._decoder._rows.values()))
    assert P._decoder.w4 and not P._decoder.w8 and rows.dec is P._decoder and rows.attn_rows == (model == "phi3")
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("B", [2, 5, 16])
def test_greedy_batched_equals_sequential(cuda, monkeypatch, model, B):
    P, cfg, tw = _llm(cuda, model)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None        # noqa: E731  a forced [SEG] from the suffix prefill's row and from decode rows
    ref, got = _both(monkeypatch, P, cfg, tw, _prompts(B), 8, hook=hook)
    _same(ref, got)
    assert all(len(e) == 2 for e in got[1])
    rows = _rows(P, model)
    assert rows.B == (2 if B == 2 else 8 if B == 5 else 16) and rows.steps == 7


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_seventeen_prompts_in_groups_of_sixteen(cuda, monkeypatch, model):
    P, cfg, tw = _llm(cuda, model)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None        # noqa: E731
    ids = _prompts(17, 6)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, ids, 8, hook=hook)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    P._decoder._rows = {}
    a = _run(P, cfg, tw, ids[:16], 8, hook=hook)
    rows = _rows(P, model)
    assert rows.B == 16 and rows.steps == 7
    b = _run(P, cfg, tw, ids[16:], 8, hook=hook)                # one prompt: the single-row mxfp4 step
    _same(ref, (a[0] + b[0], a[1] + b[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_eos_at_different_steps(cuda, monkeypatch, model):
    P, cfg, tw = _llm(cuda, model)
    ids = _prompts(6, 2)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    free, _ = _run(P, cfg, tw, ids, 12)
    eos = sorted({o[len(x) + 1 + b % 6] for b, (o, x) in enumerate(zip(free, ids))})
    ref, got = _both(monkeypatch, P, cfg, tw, ids, 12, eos=eos)
    _same(ref, got)
    assert len({len(o) - len(x) for o, x in zip(got[0], ids)}) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("k", [20, 0])          # fast route (1 <= k <= 64) / general route
def test_sampled_batched_equals_sequential(cuda, monkeypatch, model, k):
    B = 5
    P, cfg, tw = _llm(cuda, model)
    sp = [dict(T=0.8, k=k, p=0.9, seed=100 + b) for b in range(B)]
    traces_a, traces_b = [{} for _ in range(B)], [{} for _ in range(B)]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp, traces=traces_a)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp, traces=traces_b)
    _same(ref, got)
    assert traces_a == traces_b
    assert _rows(P, model).route == ("sample_fast" if k else "sample")


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(MODELS))
def test_graph_replay_equals_eager(cuda, monkeypatch, model):
    """the captured step against the eager one; the eager step is also counted: per step two MXFP4 B-row GEMVs per layer, one fp8 B-row GEMV (the
    lm_head), and the bf16 B-row GEMV only for the attention projections"""
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, tw = _llm(cuda, model)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step == 3 else None             # noqa: E731
    ids = _prompts(5, 4)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    a = _run(P, cfg, tw, ids, 8, hook=hook)
    assert _rows(P, model).graphs
    P._decoder = LlamaDecoder(P, cfg["llm"], 1024, use_graph=False)
    calls = {"w4": 0, "w8": 0, "bf16": 0}
    w4_rows, w8_rows, bf16_rows = ops.decode_gemv_w4_rows, ops.decode_gemv_w8_rows, ops.decode_gemv_rows
    monkeypatch.setattr(ops, "decode_gemv_w4_rows", lambda *x, **kw: (calls.__setitem__("w4", calls["w4"] + 1), w4_rows(*x, **kw))[1])
    monkeypatch.setattr(ops, "decode_gemv_w8_rows", lambda *x, **kw: (calls.__setitem__("w8", calls["w8"] + 1), w8_rows(*x, **kw))[1])
    monkeypatch.setattr(ops, "decode_gemv_rows", lambda *x, **kw: (calls.__setitem__("bf16", calls["bf16"] + 1), bf16_rows(*x, **kw))[1])
    b = _run(P, cfg, tw, ids, 8, hook=hook)
    rows = _rows(P, model)
    assert not rows.graphs
    _same(a, b)
    layers = cfg["llm"]["num_layers"]
    assert calls["w4"] == rows.steps * 2 * layers
    assert calls["w8"] == rows.steps
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
    assert rows.dec.w4 and rows.B == 8 and rows.steps == max(gen) - 1 and rows.steps < sum(gen) - len(gen)


# ------------------------------------------------------------------ the façade: inference_prompts(..., shared=)
def _micro(cuda, decode_weights):
    """the micro model, clip, prompts and forced [SEG] hook of test_mxfp4_gpu.py::_facade -> (model, clip, ids, rest)"""
    from videoglamm_amd import synth
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    cfg = _cfg()
    if decode_weights:
        cfg["llm"] = dict(cfg["llm"], decode_weights=decode_weights)
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
    return m, ([images], [context], [sam]), ids, ([(256, 256)], [hw])


def _equal(a, b):
    """two inference_prompts() results: the same ids, object keys and masks, pixel for pixel"""
    (oa, sa), (ob, sb) = a, b
    assert len(oa) == len(ob) and len(sa) == len(sb)
    for x, y in zip(oa, ob):
        assert torch.equal(x.reshape(-1), y.reshape(-1))
    for x, y in zip(sa, sb):
        assert sorted(x) == sorted(y) and all(sorted(x[t]) == sorted(y[t]) for t in x)
        assert all(np.array_equal(x[t][k], y[t][k]) for t in x for k in x[t])


@pytest.mark.gpu
@pytest.mark.parametrize("video", [False, True])
def test_facade_shared_route(cuda, video, monkeypatch):
    """shared=True sends an mxfp4 model down the shared route: a batched state is built (bucket 4 for 3 prompts), the result equals the same route
    with the sequential decode (VG_PROMPTS_BATCHED=0) exactly, and the ids are inference()'s per prompt.  Against inference() the masks are printed,
    not asserted: the shared route (one SAM2 call with every prompt's objects, suffix prefills on the shared prefix) is not pixel-exact with it
    (DESIGN 8).  shared=False equals the default call of an mxfp4 model."""
    m, clip, ids, rest = _micro(cuda, "mxfp4")
    kw = dict(max_new_tokens=10, use_sam2_video_branch=video)
    ref = [m.inference(*clip, x[None], *rest, **kw) for x in ids]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    default = m.inference_prompts(*clip, ids, *rest, **kw)
    dec = m.P._decoder
    assert dec.w4 and not getattr(dec, "_rows", None)
    _equal(default, m.inference_prompts(*clip, ids, *rest, shared=False, **kw))
    assert not getattr(m.P._decoder, "_rows", None)
    got = m.inference_prompts(*clip, ids, *rest, shared=True, **kw)
    dec = m.P._decoder
    rows = next(iter(dec._rows.values()))
    steps = max(o.numel() - x.numel() for o, x in zip(got[0], ids)) - 1
    assert dec.w4 and rows.dec is dec and rows.B == 4 and rows.steps == steps > 0
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    seq = m.inference_prompts(*clip, ids, *rest, shared=True, **kw)
    assert rows.steps == steps                                  # the sequential decode did not step the batched state
    _equal(got, seq)
    out, segs = got
    for b, (o, s) in enumerate(ref):
        assert torch.equal(out[b].reshape(-1), o.reshape(-1)), b
        assert sorted(segs[b]) == sorted(s[0]) and len(s[0]) > 0 and all(sorted(segs[b][t]) == sorted(s[0][t]) for t in s[0])
        m_got, m_ref = _stack(segs[b]), _stack(s[0])
        iou = (m_got & m_ref).sum() / max((m_got | m_ref).sum(), 1)
        print(f"mxfp4 shared=True ({'video' if video else 'framewise'} branch) prompt {b}: mask IoU vs inference() {iou:.6f}, "
              f"differing pixels {int((m_got != m_ref).sum())} of {m_ref.size}")


@pytest.mark.gpu
@pytest.mark.parametrize("video", [False, True])
def test_facade_shared_false_on_bf16_equals_inference(cuda, video, monkeypatch):
    """shared=False gives a bf16 model the per-prompt calls: entry b equals inference() on prompt b, ids and masks pixel for pixel"""
    m, clip, ids, rest = _micro(cuda, None)
    kw = dict(max_new_tokens=10, use_sam2_video_branch=video)
    ref = [m.inference(*clip, x[None], *rest, **kw) for x in ids]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got = m.inference_prompts(*clip, ids, *rest, shared=False, **kw)
    assert not getattr(m.P._decoder, "_rows", None)
    _equal(got, ([o for o, _ in ref], [s[0] for _, s in ref]))
