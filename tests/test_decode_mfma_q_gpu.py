"""vg_decode_gemm_w8_rows / vg_decode_gemm_w4_rows (the B-row decode projections on v_mfma_f32_16x16x32_bf16 with fp8 / MXFP4 weights) and the decode
mode cfg["llm"]["decode_gemv"] = "mfma_q" on the GPU.

1. exact integers (tests/_exact.py, the variants of test_contraction_exact_gpu._gemv_variants): no tolerance.  MXFP4 rows whose neighbouring blocks,
   and blocks 64 apart, differ in scale, with one scale byte 0 under non-zero codes per row: a lane with a neighbour's scale or the wrong 8 k of a
   block cannot pass
2. row independence: row b of a 16-row launch is the 1-row launch on row b, whatever the other rows hold (random, +-Inf / NaN), every epilogue
3. the fused RMSNorm equals ops.rmsnorm followed by the plain call, bit for bit
4. random data against the float64 product with the dequantised weights (bound gamma_K sum |x||w|), and against the VALU rows kernel (2 gamma_K)
5. the step: clips.generate_clips / prompts.generate_prompts in the mode equal vlm.generate per clip in the mode (ids, [SEG] embeddings, final-norm
   rows), greedy and sampled, captured and eager, and again on the reused RowsDecode
6. the mode is as accurate as the default one at the same decode weights: both measured against the fp32 model, the ratio bounded
7. the mode refuses bf16 weights, an uncovered width and VG_DECODE_AHEAD before any launch"""
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
NS = (16, 48, 272, 33)     # one tile, three, more than one workgroup's worth of rows per wave slice, a ragged last tile
NORM_K = 4096              # the norm form exists up to here (vg_kernels.h)
FMTS = ("fp8", "mxfp4")


def _w8(N, K, seed):
    """[2N, K] integers as e4m3 codes with power-of-two row scales 2^0 .. 2^2 (non-negative exponents: the products stay on the unit grid 1)"""
    w = E.ints((2 * N, K), seed=seed)
    sc = E.pow2(2 * N, exps=(0, 1, 2), seed=seed + 1)
    return w, sc


def _fn8(ops):
    def fn(xx, w8, s, **kw):
        return ops.decode_gemm_w8_rows(xx, w8, s[: w8.shape[0]].contiguous(), **kw)
    return fn


def _w4_buffers(ops, cuda, N, K, seed):
    """E.mxfp4_rows packed (ops.mxfp4_pack), contiguous and inside a 0x77-filled strided buffer with guard rows; the float32 matrix they mean"""
    codes, scales, deq, _ = E.mxfp4_rows(2 * N, K, seed=seed)
    assert bool((scales == 0).any(dim=1).all())                         # a scale byte 0 under non-zero codes in every row
    rows_ = ops.mxfp4_pack(codes, scales)
    big = torch.full((2 * N + 2, rows_.shape[1] + 16), 0x77, dtype=torch.uint8)
    big[:2 * N, :rows_.shape[1]] = rows_
    return rows_.to(cuda), big.to(cuda)[:2 * N, :rows_.shape[1]], deq


# ------------------------------------------------------------------ 1. exact integers
@pytest.mark.parametrize("B", (1, 3, 16))
@pytest.mark.parametrize("K", KS)
def test_exact_integers_fp8(cuda, B, K):
    from videoglamm_amd import ops
    from videoglamm_amd._lib import VGKernelError
    assert all(ops.decode_gemm_w8_rows_supported(N, K) for N in NS)
    x, xn, nw = E.ints((B, K), seed=K + B), E.ints((B, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    fn = _fn8(ops)
    for N in NS:
        w, sc = _w8(N, K, N + K)
        codes = E.e4m3_codes(w).to(cuda)
        codes_b = E.e4m3_codes(E.poisoned(w, poison=224.0)).to(cuda)[:2 * N, :K]       # ldw = K + 16
        assert codes_b.stride(0) > K
        scd = sc.to(cuda)
        _gemv_variants(cuda, fn, BF, x, xn, nw, w * sc[:, None], (codes, scd), (codes_b, scd), N, f"decode_gemm_w8_rows B={B} N={N} K={K}", unit=1.0,
                       f32_out=True, norm=K <= NORM_K)
        if K > NORM_K:
            with pytest.raises(VGKernelError):
                fn(torch.ones(B, K, dtype=BF, device=cuda), codes[:N], scd, norm_w=torch.ones(K, device=cuda), eps=1e-5)


@pytest.mark.parametrize("B", (1, 3, 16))
@pytest.mark.parametrize("K", KS)
def test_exact_integers_mxfp4(cuda, B, K):
    from videoglamm_amd import ops
    from videoglamm_amd._lib import VGKernelError
    assert all(ops.decode_gemm_w4_rows_supported(N, K) for N in NS)
    x, xn, nw = E.ints((B, K), seed=K + B), E.ints((B, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in NS:
        wd, strided, deq = _w4_buffers(ops, cuda, N, K, N + K)
        _gemv_variants(cuda, ops.decode_gemm_w4_rows, BF, x, xn, nw, deq, (wd,), (strided,), N, f"decode_gemm_w4_rows B={B} N={N} K={K}",
                       f32_out=True, norm=K <= NORM_K)
        if K > NORM_K:
            with pytest.raises(VGKernelError):
                ops.decode_gemm_w4_rows(torch.ones(B, K, dtype=BF, device=cuda), wd[:N], norm_w=torch.ones(K, device=cuda), eps=1e-5)


def test_mxfp4_scale_byte_zero_is_a_zero_block(cuda):
    """the documented reading of scale byte 0: the block contributes nothing whatever its codes hold — here EVERY block's byte is 0 under +-6 codes"""
    from videoglamm_amd import ops
    N, K = 48, 4096
    codes = torch.full((N, K // 2), 0x7F, dtype=torch.uint8)              # +6 | -6 in every byte
    w4 = ops.mxfp4_pack(codes, torch.zeros(N, K // 32, dtype=torch.uint8)).to(cuda)
    x = E.ints((3, K), seed=5).to(cuda, BF)
    y = ops.decode_gemm_w4_rows(x, w4, out_dtype=F32)
    assert torch.equal(y, torch.zeros(3, N, device=cuda))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B", (1, 3, 16))
@pytest.mark.parametrize("K", KS)
def test_glu_on_fixed_gate_sums(cuda, fmt, B, K):
    """test_decode_mfma_gpu.test_glu_on_fixed_gate_sums on the quantised kernels: gate sums that are small integers by construction (x[b] = m_b s,
    gate row n = s x a +-1 / +-2 pattern that sums to g_n in [-4, 4]), the up rows free integers; expected: ops.swiglu of the exact sums in bf16.
    All weights are in {+-1, +-2}: e4m3 codes with unit row scales, or e2m1 codes with every block scale 2^0."""
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
    if fmt == "fp8":
        y = ops.decode_gemm_w8_rows(x.to(cuda, BF), E.e4m3_codes(w).to(cuda), torch.ones(2 * N, device=cuda), glu=True)
    else:
        code = torch.where(w.abs() == 1.0, 2, 4).to(torch.uint8) | ((w < 0).to(torch.uint8) << 3)
        code = code.reshape(2 * N, K // 2, 2)
        codes = (code[..., 0] | (code[..., 1] << 4)).contiguous()
        scales = torch.full((2 * N, K // 32), 127, dtype=torch.uint8)
        assert torch.equal(ops.mxfp4_dequant(codes, scales), w)
        y = ops.decode_gemm_w4_rows(x.to(cuda, BF), ops.mxfp4_pack(codes, scales).to(cuda), glu=True)
    ref = ops.swiglu(want.to(BF).to(cuda))
    assert torch.equal(y, ref), E.explain(y, ref.cpu())


def test_exact_integers_fp8_four_tiles_per_workgroup(cuda):
    """more than 1024 tiles of 16 weight rows: the launcher gives a workgroup four tiles (the lm_head of a real vocabulary); 1025 tiles, the last
    one of a single row, leave the last workgroup one live tile of four.  fp32 output into a sentinel-guarded destination."""
    from videoglamm_amd import ops
    N, K, B = 16 * 1024 + 1, 3072, 3
    g = torch.Generator(device=cuda).manual_seed(1)
    vals = torch.tensor(E.VALS, dtype=F32, device=cuda)
    w = vals[torch.randint(4, (N, K), generator=g, device=cuda)]
    x = vals[torch.randint(4, (B, K), generator=g, device=cuda)]
    sc = torch.ldexp(torch.ones(N, device=cuda), (torch.arange(N, device=cuda) % 3).to(torch.int32))       # 1, 2, 4: neighbouring rows differ
    want = (x @ w.t()) * sc[None, :]                          # integers below 2^24: exact in fp32 in any order
    assert float((x.abs() @ w.abs().t() * sc[None, :]).max()) < E.LIMIT
    codes = w.to(torch.float8_e4m3fn)
    assert torch.equal(codes.float(), w)
    big, out = E.sentinel_out(B, N, F32, cuda)
    ops.decode_gemm_w8_rows(x.to(BF), codes.view(torch.uint8), sc, out=out)
    assert torch.equal(out, want), E.explain(out, want.cpu())
    assert E.sentinel_intact(big, B, N)


# ------------------------------------------------------------------ 2. row independence
def _rand(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


def _quantised(ops, cuda, fmt, rows, K, seed):
    """random [rows, K] weights of std K^-0.5 in the format: (the entry point as fn(x, **kw) on rows [:n], the VALU rows twin, the float64 matrix)"""
    w = torch.randn(rows, K, generator=torch.Generator().manual_seed(seed)) * K ** -0.5
    if fmt == "fp8":
        sc = (w.abs().amax(dim=1) / 448.0).float()
        q = (w / sc[:, None]).to(torch.float8_e4m3fn)
        deq = q.double() * sc.double()[:, None]
        w8, scd = q.view(torch.uint8).to(cuda), sc.to(cuda)
        return (lambda x, n=rows, **kw: ops.decode_gemm_w8_rows(x, w8[:n], scd[:n].contiguous(), **kw),
                lambda x, n=rows, **kw: ops.decode_gemv_w8_rows(x, w8[:n], scd[:n].contiguous(), **kw), deq)
    codes, scales = ops.quantize_mxfp4_rows(w)
    w4 = ops.mxfp4_pack(codes, scales).to(cuda)
    return (lambda x, n=rows, **kw: ops.decode_gemm_w4_rows(x, w4[:n], **kw), lambda x, n=rows, **kw: ops.decode_gemv_w4_rows(x, w4[:n], **kw),
            ops.mxfp4_dequant(codes, scales).double())


def _epilogues(K, N, cuda):
    nw = (torch.rand(K, generator=torch.Generator().manual_seed(9)) + 0.5).to(cuda)
    res = {dt: _rand((16, N), 11).to(dt).to(cuda) for dt in (BF, F32)}
    eps = [("plain", {}, None), ("residual", {}, BF), ("fp32 out", dict(out_dtype=F32), None), ("fp32 out + residual", dict(out_dtype=F32), F32),
           ("glu", dict(glu=True), None), ("glu fp32 out", dict(glu=True, out_dtype=F32), None)]
    if K <= NORM_K:
        eps += [("norm", dict(norm_w=nw, eps=1e-5), None), ("norm + glu", dict(norm_w=nw, eps=1e-5, glu=True), None),
                ("norm + residual, fp32 out", dict(norm_w=nw, eps=1e-5, out_dtype=F32), F32)]
    return eps, res


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", KS)
def test_row_independence(cuda, fmt, K):
    from videoglamm_amd import ops
    N = 272
    fn, _, _ = _quantised(ops, cuda, fmt, 2 * N, K, K)
    x = _rand((16, K), K + 1, 2.0).to(cuda)
    bad = torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=BF, device=cuda)
    eps, res = _epilogues(K, N, cuda)
    for name, kw, rdt in eps:
        n = 2 * N if kw.get("glu") else N
        r = None if rdt is None else res[rdt]
        y16 = fn(x, n, residual=r, **kw)
        assert bool(torch.isfinite(y16).all()) and float(y16.float().abs().max()) > 0
        for b in range(16):
            y1 = fn(x[b:b + 1], n, residual=None if r is None else r[b:b + 1], **kw)
            assert torch.equal(y16[b:b + 1], y1), (name, K, b)
        y5 = fn(x[:5], n, residual=None if r is None else r[:5], **kw)
        assert torch.equal(y5, y16[:5]), (name, K, "B = 5")
        for b in (0, 6, 15):                                 # the other 15 rows hold +-Inf / NaN
            xp = bad[torch.arange(16 * K, device=cuda) % 3].view(16, K).clone()
            xp[b] = x[b]
            yp = fn(xp, n, residual=r, **kw)
            assert torch.equal(yp[b], y16[b]), (name, K, b, "poisoned neighbours")
            assert not bool(torch.isfinite(yp[(b + 1) % 16]).any())


# ------------------------------------------------------------------ 3. fused norm = ops.rmsnorm, then the plain call
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B", (1, 16))
@pytest.mark.parametrize("K", (3072, 4096))
def test_fused_norm_equals_rmsnorm_then_plain(cuda, fmt, B, K):
    from videoglamm_amd import ops
    N = 272
    fn, _, _ = _quantised(ops, cuda, fmt, 2 * N, K, K)
    x = _rand((B, K), K + B, 3.0).to(cuda)
    nw = (torch.rand(K, generator=torch.Generator().manual_seed(2)) + 0.5).to(cuda)
    h = ops.rmsnorm(x, nw, 1e-5)
    assert torch.equal(fn(x, N, norm_w=nw, eps=1e-5), fn(h, N))
    assert torch.equal(fn(x, 2 * N, norm_w=nw, eps=1e-5, glu=True), fn(h, 2 * N, glu=True))
    assert torch.equal(fn(x, N, norm_w=nw, eps=1e-5, out_dtype=F32), fn(h, N, out_dtype=F32))


# ------------------------------------------------------------------ 4. random data against the float64 product
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,K", [(272, 14336), (1001, 8192), (1001, 4096), (2064, 3072)])
def test_random_against_float64(cuda, fmt, N, K):
    """fp32 out against the float64 product with the dequantised weights (ops.mxfp4_dequant; scale x e4m3).  MXFP4: K exact products (a scaled
    e2m1 value is a bf16) summed in fp32 in some order: |err| <= gamma_K sum_k |x_k w_k|, gamma_K = K u / (1 - K u), u = 2^-24 (Higham, eq. 3.5).
    fp8: the K exact products x_k q_k are summed the same way and the total is multiplied once by the fp32 row scale, which the reference holds as
    the same fp32 number; the bound stays gamma_K (the measured ratio, printed, is two orders below it).
    Against the VALU rows kernel on the same operands: two sums of the same exact products in two orders, 2 gamma_K sum |x||w|."""
    from videoglamm_amd import ops
    fn, valu, deq = _quantised(ops, cuda, fmt, N, K, N + K)
    x = (torch.randn(16, K, generator=torch.Generator().manual_seed(N)) * 2.0).to(BF)
    ref = x.double() @ deq.t()
    mag = x.double().abs() @ deq.abs().t()
    u = 2.0 ** -24
    gamma = K * u / (1 - K * u)
    y32 = fn(x.to(cuda), out_dtype=F32).double().cpu()
    err = (y32 - ref).abs()
    print(f"{fmt} N={N} K={K}: max err / bound = {float((err / (gamma * mag)).max()):.4f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= gamma * mag).all())
    yv = valu(x.to(cuda), out_dtype=F32).double().cpu()
    d = (y32 - yv).abs()
    print(f"   against the VALU rows kernel: max |d| / (2 gamma sum|x||w|) = {float((d / (2 * gamma * mag)).max()):.4f}")
    assert bool((d <= 2 * gamma * mag).all())


# ------------------------------------------------------------------ 5. the step
MODELS = [("llama", "fp8"), ("llama", "mxfp4"), ("phi3", "fp8"), ("phi3", "mxfp4")]


def _llm(cuda, model, dw, **llm_kw):
    P, cfg, tw = (phi3 if model == "phi3" else llama)._llm(cuda)
    return P, dict(cfg, llm=dict(cfg["llm"], decode_gemv="mfma_q", decode_weights=dw, **llm_kw)), tw


def _alone(P, cfg, text, visuals, n, hook, sp):
    """vlm.generate per clip: (ids, [SEG] embeddings, the final-norm rows of the prompt and of every decode step)"""
    from videoglamm_amd import vlm
    out = []
    for b, (_, _, ids) in enumerate(text):
        o, e = vlm.generate(P, cfg, None, None, None, ids, n, None, visual=visuals[b], token_hook=hook, sampling=None if sp is None else sp[b])
        S = ids.numel() - 4 + visuals[b].shape[0]
        out.append((o, e.clone(), P._decoder.hid_all[:S + n - 1].clone()))
    assert P._decoder.mfma_q and not P._decoder.mfma
    return out


def _batched(P, cfg, text, visuals, n, hook, sp):
    got = tc._batched(P, cfg, text, visuals, n, hook=hook, samplings=sp)
    rows = tc._rows(P)
    assert rows.dec.mfma_q and not rows.dec.mfma
    return [(o, e, rows.hid[j, :t[2].numel() - 4 + v.shape[0] + n - 1].clone()) for j, ((o, e), t, v) in enumerate(zip(got, text, visuals))]


def _same(got, ref):
    assert len(got) == len(ref)
    for b, ((o, e, h), (ro, re, rh)) in enumerate(zip(got, ref)):
        assert torch.equal(o, ro), (b, o.tolist(), ro.tolist())
        assert e.shape == re.shape and torch.equal(e, re), b
        assert h.shape == rh.shape and torch.equal(h, rh), b


@pytest.mark.parametrize("model,dw", MODELS)
def test_generate_clips_equals_generate_in_the_mode(cuda, model, dw):
    """greedy and sampled on the captured step, then the reused RowsDecode, then eager — with the kernels each projection runs on counted"""
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = _llm(cuda, model, dw)
    B = 5                                                     # a bucket of 8: three padded rows
    text, visuals = tc._make(cfg, cuda, B, seed=B)
    pos = [t[2].numel() - 4 + v.shape[0] for t, v in zip(text, visuals)]
    assert min(pos) < 256 <= max(pos)                      # rows on both sides of a 256-key block edge
    hook = tc.SEG_HOOK(cfg["seg_token_idx"])
    first = {}
    for mode in ("greedy", "k20"):
        sp = tc._sampling(mode, B)
        ref = _alone(P, cfg, text, visuals, 8, hook, sp)
        got = _batched(P, cfg, text, visuals, 8, hook, sp)
        _same(got, ref)
        assert all(e.shape == (2, 256) for _, e, _ in got)
        first[mode] = got
    rows = tc._rows(P)
    assert rows.attn_rows == (model == "phi3") and sorted(rows.graphs) == ["greedy", "sample_fast"]
    again = _batched(P, cfg, text, visuals, 8, hook, None)   # the reused RowsDecode and its captured graph
    assert tc._rows(P) is rows
    _same(again, first["greedy"])
    # eager, and which kernels the step calls: never a VALU GEMV
    calls = {}

    def count(name):
        fn = getattr(ops, name)

        def wrapped(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        return wrapped
    names = ["decode_gemm_rows", "decode_gemm_w8_rows", "decode_gemm_w4_rows", "decode_gemv_rows", "decode_gemv_w8_rows", "decode_gemv_w4_rows",
             "decode_gemv", "decode_gemv_w8", "decode_gemv_w4"]
    mp = pytest.MonkeyPatch()
    try:
        for nm in names:
            mp.setattr(ops, nm, count(nm))
        P._decoder = LlamaDecoder(P, cfg["llm"], 1024, use_graph=False)
        eager = _batched(P, cfg, text, visuals, 8, hook, None)
    finally:
        mp.undo()
    assert not tc._rows(P).graphs
    _same(eager, first["greedy"])
    steps, bf16_per_layer = 7, 2 if model == "phi3" else 1       # 7 steps of the bucket of 8; o (and Phi-3's q|k|v) per layer
    want = {"decode_gemm_rows": steps * 2 * bf16_per_layer}
    if dw == "fp8":
        want["decode_gemm_w8_rows"] = steps * (2 * 2 + 1) + B      # gate|up and down of two layers and the lm_head; B single-row lm_heads
    else:
        want["decode_gemm_w4_rows"] = steps * 2 * 2
        want["decode_gemm_w8_rows"] = steps + B
    assert calls == want, calls


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("model,dw", MODELS)
def test_generate_prompts_on_the_shared_route_in_the_mode(cuda, monkeypatch, model, dw, B):
    """prompts.generate_prompts on the batched step (B = 2: a full bucket; B = 5: a bucket of 8 with three padded rows) equals its sequential loop,
    which runs the mode's single-row step: ids and [SEG] embeddings, greedy and sampled"""
    mod = phi3 if model == "phi3" else llama
    P, cfg, tw = _llm(cuda, model, dw)
    ids = mod._prompts(B, seed=B)
    hook = tc.SEG_HOOK(cfg["seg_token_idx"])
    for sp in (None, [dict(T=0.8, k=20, p=0.9, seed=100 + b) for b in range(B)]):
        ref, got = mod._both(monkeypatch, P, cfg, tw, ids, 7, hook=hook, samplings=sp)
        mod._same(ref, got)
        assert len(set(map(tuple, got[0]))) > 1
    dec = P._decoder
    assert dec.mfma_q and len(dec._rows) == 1 and next(iter(dec._rows.values())).steps > 0


# ------------------------------------------------------------------ 6. as accurate as the default mode at the same decode weights
@pytest.mark.parametrize("model,dw", MODELS)
def test_accuracy_calibrated_against_the_default_mode(cuda, model, dw):
    """The scheme of test_decode_mfma_gpu's test 6: teacher-forced over seven decode steps after a 40-row prefill, the final-norm row of every step
    against the fp32 model holding the same (bf16-representable) weights: e = max over the rows of max |row - ref| / max |ref|.  The mode and the
    default mode hold the SAME quantised weights and round at the same points; they differ only in the fp32 summation order, so
    e_mfma_q <= 1.5 e_valu (the project's factor for two such paths), and the lm_head's argmax equals the fp32 model's wherever the default mode's does.
    Measured on an MI355X (the figures are printed): Llama width fp8 e_valu 0.06220, e_mfma_q 0.06177; mxfp4 0.25367, 0.25452;
    Phi-3 width fp8 0.07358, 0.07358; mxfp4 0.31615, 0.31726; the mode's argmax equal to the default mode's at every step."""
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
        assert dec.mfma_q == (llm_kw.get("decode_gemv") == "mfma_q") and not dec.mfma
        dec.reset()
        dec.forward(x.to(cuda, dtype))
        rows, arg = [], []
        for t in range(steps):
            dec.tok_dev.fill_(forced[t])
            dec.decode_step()
            h = dec.hid_all[S + t:S + t + 1].clone()
            rows.append(h.float())
            if dec.mfma_q:
                logits = ops.decode_gemm_w8_rows(h, *P.fp8("lm_head"), out_dtype=F32)
            elif dec.w8 or dec.w4:
                logits = ops.decode_gemv_w8(h, *P.fp8("lm_head"), out_dtype=F32)
            else:
                logits = ops.linear(h, P.w("lm_head"), out_dtype=F32)
            arg.append(int(logits.view(-1).argmax()))
        return torch.cat(rows), arg

    ref, aref = run(F32, {})
    valu, avalu = run(BF, dict(decode_weights=dw))
    mq, amq = run(BF, dict(decode_weights=dw, decode_gemv="mfma_q"))
    err = lambda y: float(((y - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)).max())      # noqa: E731
    e_valu, e_mq = err(valu), err(mq)
    print(f"{model} {dw}: e_valu = {e_valu:.5f}  e_mfma_q = {e_mq:.5f}  argmax fp32 {aref} valu {avalu} mfma_q {amq}")
    assert e_valu > 0 and e_mq <= 1.5 * e_valu
    assert all(m == r for m, v, r in zip(amq, avalu, aref) if v == r)


# ------------------------------------------------------------------ 7. refusals on the device path
def test_mode_refused_before_any_launch(cuda, monkeypatch):
    from videoglamm_amd import ops
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder

    def no_launch(*a, **kw):
        raise AssertionError("a launch in a refused mode")
    for nm in ("decode_gemm_rows", "decode_gemm_w8_rows", "decode_gemm_w4_rows"):
        monkeypatch.setattr(ops, nm, no_launch)
    # bf16 weights: the message points to "mfma"
    P, cfg, _ = llama._llm(cuda)
    cfg = dict(cfg, llm=dict(cfg["llm"], decode_gemv="mfma_q"))
    with pytest.raises(ValueError, match="'mfma'"):
        LlamaDecoder(P, cfg["llm"], 1024)
    text, visuals = tc._make(cfg, cuda, 2)
    with pytest.raises(ValueError, match="'mfma'"):
        tc._batched(P, cfg, text, visuals, 4)
    # an uncovered width: an MLP of 11008 columns (a K the kernels do not walk)
    c, sd = llama._weights()
    sd = {k: (v.to(BF) if v.dim() >= 2 else v) for k, v in sd.items()}
    for k in list(sd):
        if k.endswith(("gate_proj.weight", "up_proj.weight")):
            sd[k] = sd[k][:11008].contiguous()
        elif k.endswith("down_proj.weight"):
            sd[k] = sd[k][:, :11008].contiguous()
    c = dict(c, ffn=11008) if "ffn" in c else c
    P2 = Params(sd, cuda, BF)
    for dw in FMTS:
        with pytest.raises((ValueError, AssertionError), match="11008|row lengths"):
            LlamaDecoder(P2, dict(c, decode_gemv="mfma_q", decode_weights=dw), 1024)
    # VG_DECODE_AHEAD
    monkeypatch.setenv("VG_DECODE_AHEAD", "1")
    P3, cfg3, _ = _llm(cuda, "llama", "fp8")
    with pytest.raises(ValueError, match="VG_DECODE_AHEAD"):
        LlamaDecoder(P3, cfg3["llm"], 1024)
    with pytest.raises(ValueError, match="VG_DECODE_AHEAD"):
        tc._batched(P3, cfg3, text, visuals, 4)
