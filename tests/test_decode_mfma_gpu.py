"""vg_decode_gemm_rows (the B-row decode projections on v_mfma_f32_16x16x32_bf16) and the decode mode cfg["llm"]["decode_gemv"] = "mfma" on the
GPU.

1. exact integers (tests/_exact.py, the variants of test_contraction_exact_gpu._gemv_variants): no tolerance
2. row independence: row b of a 16-row launch is the 1-row launch on row b, whatever the other rows hold (random, +-Inf / NaN), every epilogue
3. the fused RMSNorm equals ops.rmsnorm followed by the plain call, bit for bit
4. random data against the float64 product, the bound derived: K products in fp32, any order -> gamma_K = K u / (1 - K u), u = 2^-24
5. the step: clips.generate_clips in the mode equals vlm.generate per clip in the mode (ids, [SEG] embeddings, final-norm rows), greedy and
   sampled, captured and eager, and again on the reused RowsDecode
6. the mode is as accurate as the default one: both measured against the fp32 model, the ratio bounded
7. the mode refuses fp8 / mxfp4 decode weights and an uncovered width before any launch"""
import pytest
import torch

import _exact as E
import test_clips_gpu as tc
import test_prompts_batched_gpu as llama
import test_prompts_batched_phi3_gpu as phi3
from test_contraction_exact_gpu import _gemv_variants

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BF, F32 = torch.bfloat16, torch.float32
KS = (3072, 4096, 8192, 14336)
NORM_K = 4096            # the norm form exists up to here (vg_kernels.h)


# ------------------------------------------------------------------ 1. exact integers
@pytest.mark.parametrize("B", (1, 3, 16))
@pytest.mark.parametrize("K", KS)
def test_exact_integers(cuda, B, K):
    from videoglamm_amd import ops
    from videoglamm_amd._lib import VGKernelError
    x, xn, nw = E.ints((B, K), seed=K + B), E.ints((B, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in (16, 48, 272, 33):                              # (33: a ragged last tile, as a vocabulary with added tokens has)
        w = E.ints((2 * N, K), seed=N + K)
        wb = E.poisoned(w, dtype=BF).to(cuda)[:2 * N, :K]
        _gemv_variants(cuda, ops.decode_gemm_rows, BF, x, xn, nw, w, (w.to(cuda, BF),), (wb,), N, f"decode_gemm_rows B={B} N={N} K={K}",
                       f32_out=True, norm=K <= NORM_K)
        if K > NORM_K:
            with pytest.raises(VGKernelError):
                ops.decode_gemm_rows(torch.ones(B, K, dtype=BF, device=cuda), wb[:N], norm_w=torch.ones(K, device=cuda), eps=1e-5)


@pytest.mark.parametrize("B", (1, 3, 16))
@pytest.mark.parametrize("K", KS)
def test_glu_on_fixed_gate_sums(cuda, B, K):
    """gate sums that are small integers by construction: x[b] = m_b s (s a sign pattern), gate row n = s x (+1, -1, +1, -1, ...) with its first
    |g_n| signs set to sign(g_n), so row n sums to g_n in [-4, 4] and the gate of (b, n) is m_b g_n; the up rows are free integers.  Expected:
    ops.swiglu (the one vg_silu table) of the exact gate | up sums rounded to bf16."""
    from videoglamm_amd import ops
    N = 48
    s = E.ints((K,), (-1, 1), seed=K)
    m = E.ints((B,), (-2, -1, 1, 2), seed=B)
    x = m[:, None] * s[None, :]
    g = (torch.arange(N) % 9 - 4).float()
    c = torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0)[None, :].repeat(N, 1)
    for n in range(N):                                      # an even prefix that sums to g_n; the alternating tail behind it sums to 0
        a, sg = int(abs(g[n])), float(torch.sign(g[n]))
        if a % 2 == 0:
            c[n, :a] = sg
        elif a == 1:
            c[n, 0], c[n, 1] = 2 * sg, -sg
        else:
            c[n, 0], c[n, 1:a - 1] = 2 * sg, sg
    wg = c * s[None, :]
    gate = x @ wg.t()
    assert bool((gate.abs() <= 8).all()) and gate.abs().max() >= 4 and len(gate.unique()) >= 5
    w = torch.cat([wg, E.ints((N, K), seed=K + 7)])
    want = E.reference(x, w)                                  # [B, 2N] exact
    assert torch.equal(want[:, :N], gate)
    y = ops.decode_gemm_rows(x.to(cuda, BF), w.to(cuda, BF), glu=True)
    ref = ops.swiglu(want.to(BF).to(cuda))
    assert torch.equal(y, ref), E.explain(y, ref.cpu())


def test_exact_integers_four_tiles_per_workgroup(cuda):
    """more than 1024 tiles of 16 weight rows: the launcher gives a workgroup four tiles (the lm_head of a real vocabulary); 1025 tiles, the last
    one of a single row, leave the last workgroup one live tile of four"""
    from videoglamm_amd import ops
    N, K, B = 16 * 1024 + 1, 3072, 3
    g = torch.Generator(device=cuda).manual_seed(1)
    vals = torch.tensor(E.VALS, dtype=BF, device=cuda)
    w = vals[torch.randint(4, (N, K), generator=g, device=cuda)]
    x = vals[torch.randint(4, (B, K), generator=g, device=cuda)]
    want = x.float() @ w.float().t()                         # integers below 2^24: exact in fp32 in any order
    assert float((x.float().abs() @ w.float().abs().t()).max()) < E.LIMIT
    big, out = E.sentinel_out(B, N, F32, cuda)
    ops.decode_gemm_rows(x, w, out=out)
    assert torch.equal(out, want) and E.sentinel_intact(big, B, N)
    assert torch.equal(ops.decode_gemm_rows(x, w), want.to(BF))


# ------------------------------------------------------------------ 2. row independence
def _rand(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


def _epilogues(K, N, cuda):
    nw = (torch.rand(K, generator=torch.Generator().manual_seed(9)) + 0.5).to(cuda)
    res = {dt: _rand((16, N), 11).to(dt).to(cuda) for dt in (BF, F32)}
    eps = [("plain", {}, None), ("residual", {}, BF), ("fp32 out", dict(out_dtype=F32), None), ("fp32 out + residual", dict(out_dtype=F32), F32),
           ("glu", dict(glu=True), None), ("glu fp32 out", dict(glu=True, out_dtype=F32), None)]
    if K <= NORM_K:
        eps += [("norm", dict(norm_w=nw, eps=1e-5), None), ("norm + glu", dict(norm_w=nw, eps=1e-5, glu=True), None),
                ("norm + residual, fp32 out", dict(norm_w=nw, eps=1e-5, out_dtype=F32), F32)]
    return eps, res


@pytest.mark.parametrize("K", KS)
def test_row_independence(cuda, K):
    from videoglamm_amd import ops
    N = 272
    w = _rand((2 * N, K), K, 0.05).to(cuda)
    x = _rand((16, K), K + 1, 2.0).to(cuda)
    bad = torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=BF, device=cuda)
    eps, res = _epilogues(K, N, cuda)
    for name, kw, rdt in eps:
        wm = w if kw.get("glu") else w[:N]
        r = None if rdt is None else res[rdt]
        y16 = ops.decode_gemm_rows(x, wm, residual=r, **kw)
        assert bool(torch.isfinite(y16).all()) and float(y16.float().abs().max()) > 0
        for b in range(16):
            y1 = ops.decode_gemm_rows(x[b:b + 1], wm, residual=None if r is None else r[b:b + 1], **kw)
            assert torch.equal(y16[b:b + 1], y1), (name, K, b)
        y5 = ops.decode_gemm_rows(x[:5], wm, residual=None if r is None else r[:5], **kw)
        assert torch.equal(y5, y16[:5]), (name, K, "B = 5")
        for b in (0, 6, 15):                                 # the other 15 rows hold +-Inf / NaN
            xp = bad[torch.arange(16 * K, device=cuda) % 3].view(16, K).clone()
            xp[b] = x[b]
            yp = ops.decode_gemm_rows(xp, wm, residual=r, **kw)
            assert torch.equal(yp[b], y16[b]), (name, K, b, "poisoned neighbours")
            assert not bool(torch.isfinite(yp[(b + 1) % 16]).any())


# ------------------------------------------------------------------ 3. fused norm = ops.rmsnorm, then the plain call
@pytest.mark.parametrize("B", (1, 16))
@pytest.mark.parametrize("K", (3072, 4096))
def test_fused_norm_equals_rmsnorm_then_plain(cuda, B, K):
    from videoglamm_amd import ops
    N = 272
    w = _rand((2 * N, K), K, 0.05).to(cuda)
    x = _rand((B, K), K + B, 3.0).to(cuda)
    nw = (torch.rand(K, generator=torch.Generator().manual_seed(2)) + 0.5).to(cuda)
    h = ops.rmsnorm(x, nw, 1e-5)
    assert torch.equal(ops.decode_gemm_rows(x, w[:N], norm_w=nw, eps=1e-5), ops.decode_gemm_rows(h, w[:N]))
    assert torch.equal(ops.decode_gemm_rows(x, w, norm_w=nw, eps=1e-5, glu=True), ops.decode_gemm_rows(h, w, glu=True))
    assert torch.equal(ops.decode_gemm_rows(x, w[:N], norm_w=nw, eps=1e-5, out_dtype=F32), ops.decode_gemm_rows(h, w[:N], out_dtype=F32))


# ------------------------------------------------------------------ 4. random data against the float64 product
@pytest.mark.parametrize("N,K", [(272, 14336), (9216, 3072)])
def test_random_against_float64(cuda, N, K):
    """fp32 out: K exact bf16 x bf16 products summed in fp32 in some order: |err| <= gamma_K sum_k |x_k w_k|, gamma_K = K u / (1 - K u), u = 2^-24
    (Higham, Accuracy and Stability, eq. 3.5; the float64 reference's own error, ~K 2^-53, is nine orders below it).  bf16 out: the one rounding
    of a value inside that interval, and rounding is monotone: RNE(lo) <= y <= RNE(hi), lo / hi widened by the float32 step the conversion takes."""
    from videoglamm_amd import ops
    g = torch.Generator(device=cuda).manual_seed(N)
    w = (torch.randn(N, K, generator=g, device=cuda) * 0.05).to(BF)
    x = (torch.randn(16, K, generator=g, device=cuda) * 2.0).to(BF)
    ref = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    u = 2.0 ** -24
    bound = (K * u / (1 - K * u)) * mag
    y32 = ops.decode_gemm_rows(x, w, out_dtype=F32)
    err = (y32.double() - ref).abs()
    print(f"N={N} K={K}: max err / bound = {float((err / bound).max()):.4f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= bound).all())
    y16 = ops.decode_gemm_rows(x, w).double()
    slack = ref.abs() * 2.0 ** -23
    lo, hi = (ref - bound - slack).float().to(BF).double(), (ref + bound + slack).float().to(BF).double()
    assert bool(((y16 >= lo) & (y16 <= hi)).all())


# ------------------------------------------------------------------ 5. the step
def _llm(cuda, model, **llm_kw):
    P, cfg, _ = (phi3 if model == "phi3" else llama)._llm(cuda)
    return P, dict(cfg, llm=dict(cfg["llm"], decode_gemv="mfma", **llm_kw))


def _alone(P, cfg, text, visuals, n, hook, sp):
    """vlm.generate per clip: (ids, [SEG] embeddings, the final-norm rows of the prompt and of every decode step)"""
    from videoglamm_amd import vlm
    out = []
    for b, (_, _, ids) in enumerate(text):
        o, e = vlm.generate(P, cfg, None, None, None, ids, n, None, visual=visuals[b], token_hook=hook, sampling=None if sp is None else sp[b])
        S = ids.numel() - 4 + visuals[b].shape[0]
        out.append((o, e.clone(), P._decoder.hid_all[:S + n - 1].clone()))
    assert P._decoder.mfma
    return out


def _batched(P, cfg, text, visuals, n, hook, sp):
    got = tc._batched(P, cfg, text, visuals, n, hook=hook, samplings=sp)
    rows = tc._rows(P)
    assert rows.dec.mfma
    return [(o, e, rows.hid[j, :t[2].numel() - 4 + v.shape[0] + n - 1].clone()) for j, ((o, e), t, v) in enumerate(zip(got, text, visuals))]


def _same(got, ref):
    assert len(got) == len(ref)
    for b, ((o, e, h), (ro, re, rh)) in enumerate(zip(got, ref)):
        assert torch.equal(o, ro), (b, o.tolist(), ro.tolist())
        assert e.shape == re.shape and torch.equal(e, re), b
        assert h.shape == rh.shape and torch.equal(h, rh), b


@pytest.mark.parametrize("B", [2, 5, 16])
@pytest.mark.parametrize("model", ["llama", "phi3"])
def test_generate_clips_equals_generate_in_the_mode(cuda, model, B):
    P, cfg = _llm(cuda, model)
    text, visuals = tc._make(cfg, cuda, B, seed=B)
    pos = [t[2].numel() - 4 + v.shape[0] for t, v in zip(text, visuals)]
    assert min(pos) < 256 <= max(pos)                      # rows on both sides of a 256-key block edge
    hook = tc.SEG_HOOK(cfg["seg_token_idx"])
    for mode in ("greedy", "k20"):
        sp = tc._sampling(mode, B)
        ref = _alone(P, cfg, text, visuals, 9, hook, sp)
        got = _batched(P, cfg, text, visuals, 9, hook, sp)
        _same(got, ref)
        assert all(e.shape == (2, 256) for _, e, _ in got)
    rows = tc._rows(P)
    assert rows.attn_rows == (model == "phi3") and sorted(rows.graphs) == ["greedy", "sample_fast"]


@pytest.mark.parametrize("model", ["llama", "phi3"])
def test_captured_equals_eager_and_the_second_call_the_first(cuda, model, monkeypatch):
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg = _llm(cuda, model)
    text, visuals = tc._make(cfg, cuda, 5, seed=8)
    hook = tc.SEG_HOOK(cfg["seg_token_idx"])
    a = _batched(P, cfg, text, visuals, 8, hook, None)
    rows = tc._rows(P)
    assert sorted(rows.graphs) == ["greedy"]
    a2 = _batched(P, cfg, text, visuals, 8, hook, None)      # the reused RowsDecode and its captured graph
    assert tc._rows(P) is rows and rows.steps == 14
    _same(a2, a)
    # eager, and which kernels the step calls: the MFMA projection for every plain GEMV and the lm_head, never the VALU rows kernel or the skinny GEMM
    calls = {"mfma": 0, "valu": 0, "skinny16": 0}
    gemm_rows, gemv_rows, linear = ops.decode_gemm_rows, ops.decode_gemv_rows, ops.linear
    monkeypatch.setattr(ops, "decode_gemm_rows", lambda *x, **kw: (calls.__setitem__("mfma", calls["mfma"] + 1), gemm_rows(*x, **kw))[1])
    monkeypatch.setattr(ops, "decode_gemv_rows", lambda *x, **kw: (calls.__setitem__("valu", calls["valu"] + 1), gemv_rows(*x, **kw))[1])
    monkeypatch.setattr(ops, "linear", lambda x, w, *a_, **kw: (calls.__setitem__("skinny16", calls["skinny16"] + (w.shape[0] == 8192 and x.shape[0] == 8)),
                                                              linear(x, w, *a_, **kw))[1])
    P._decoder = LlamaDecoder(P, cfg["llm"], 1024, use_graph=False)
    b = _batched(P, cfg, text, visuals, 8, hook, None)
    assert not tc._rows(P).graphs
    _same(b, a)
    per_layer = 4 if model == "phi3" else 3
    assert calls == {"mfma": 7 * (2 * per_layer + 1) + 5, "valu": 0, "skinny16": 0}, calls      # 7 steps of the bucket of 8; 5 single-row lm_heads


# ------------------------------------------------------------------ 6. as accurate as the default mode
@pytest.mark.parametrize("model", ["llama", "phi3"])
def test_accuracy_calibrated_against_the_default_mode(cuda, model):
    """Teacher-forced over seven decode steps after a 40-row prefill, the final-norm row of every step against the fp32 model holding the same
    (bf16-representable) weights: e = max over the rows of max |row - ref| / max |ref|.  The two modes round at the same points and differ only in
    the fp32 summation order, so e_mfma <= 1.5 e_valu (the factor: run-to-run spread of a maximum over a few thousand values), and the lm_head's
    argmax equals the fp32 model's wherever the default mode's does.
    Measured on an MI355X (the figures are printed): Llama width e_valu 0.01529, e_mfma 0.01469; Phi-3 width 0.01392,
    0.01509; every argmax equal to the fp32 model's in both modes."""
    from videoglamm_amd import ops
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    mod = phi3 if model == "phi3" else llama
    c, sd = mod._weights()
    if model == "phi3":
        c = dict(c, sliding_window=199)
    sd16 = {k: (v.to(BF) if v.dim() >= 2 else v) for k, v in sd.items()}
    g = torch.Generator().manual_seed(17)
    S, steps = 40, 7
    x = (torch.randn(S, c["hidden"], generator=g) * 0.5).to(BF)
    forced = torch.randint(10, 8000, (steps,), generator=g).tolist()

    def run(dtype, llm_kw):
        P = Params({k: v.to(dtype) if v.dim() >= 2 else v for k, v in sd16.items()}, cuda, dtype)
        dec = LlamaDecoder(P, dict(c, **llm_kw), 1024, use_graph=False)
        assert dec.mfma == (llm_kw.get("decode_gemv") == "mfma")
        dec.reset()
        dec.forward(x.to(cuda, dtype))
        rows, arg = [], []
        for t in range(steps):
            dec.tok_dev.fill_(forced[t])
            dec.decode_step()
            h = dec.hid_all[S + t:S + t + 1].clone()
            rows.append(h.float())
            logits = ops.decode_gemm_rows(h, P.w("lm_head"), out_dtype=F32) if dec.mfma else ops.linear(h, P.w("lm_head"), out_dtype=F32)
            arg.append(int(logits.view(-1).argmax()))
        return torch.cat(rows), arg

    ref, aref = run(F32, {})
    valu, avalu = run(BF, {})
    mfma, amfma = run(BF, dict(decode_gemv="mfma"))
    err = lambda y: float(((y - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)).max())      # noqa: E731
    e_valu, e_mfma = err(valu), err(mfma)
    print(f"{model}: e_valu = {e_valu:.5f}  e_mfma = {e_mfma:.5f}  argmax fp32 {aref} valu {avalu} mfma {amfma}")
    assert e_valu > 0 and e_mfma <= 1.5 * e_valu
    assert all(m == r for m, v, r in zip(amfma, avalu, aref) if v == r)


# ------------------------------------------------------------------ 7. refusals on the device path
def test_mode_refused_before_any_launch(cuda, monkeypatch):
    from videoglamm_amd import ops
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder

    def no_launch(*a, **kw):
        raise AssertionError("a launch in a refused mode")
    monkeypatch.setattr(ops, "decode_gemm_rows", no_launch)
    for dw in ("fp8", "mxfp4"):
        P, cfg = _llm(cuda, "llama", decode_weights=dw)
        with pytest.raises(ValueError, match=dw):
            LlamaDecoder(P, cfg["llm"], 1024)
        text, visuals = tc._make(cfg, cuda, 2)
        with pytest.raises(ValueError, match=dw):
            tc._batched(P, cfg, text, visuals, 4)
    # an uncovered width: an MLP of 11008 columns (a K the kernel does not walk)
    c, sd = llama._weights()
    sd = {k: (v.to(BF) if v.dim() >= 2 else v) for k, v in sd.items()}
    for k in list(sd):
        if k.endswith(("gate_proj.weight", "up_proj.weight")):
            sd[k] = sd[k][:11008].contiguous()
        elif k.endswith("down_proj.weight"):
            sd[k] = sd[k][:, :11008].contiguous()
    c = dict(c, ffn=11008) if "ffn" in c else c
    P = Params(sd, cuda, BF)
    with pytest.raises(ValueError, match="11008"):
        LlamaDecoder(P, dict(c, decode_gemv="mfma"), 1024)
    assert not LlamaDecoder(P, dict(c), 1024).mfma           # the default mode takes the same model
