"""The power of tests/test_contraction_exact_gpu.py, proved without a GPU: a blocked CPU GEMM (K steps, optional K split, fp32 accumulation, one
output rounding: tests/_exact.py) stands in for the kernel.  The honest model equals the float64 reference bit for bit on the shapes of the GPU
file's case tables (every ops.linear route, split-K, the window forms as GEMMs over the window-order rows, bmm_nt, the GEMVs and their B-row
forms, q|k|v, linear_rows, fp8 and MXFP4 operands on their scale grid, the three mlp3 layers) — whatever the K step or the split; data movement
around the GEMM (window gather / scatter, RoPE's signed swap, the A + A2 prologue) is not modelled — and every wrong kernel of _exact.MUTANTS fails the comparison, applied to every output, to one ragged
tile only, or to one output row only.  test_tolerance_gap_is_recorded shows what the exact tests add: the same mutants applied to EVERY output
pass the K-scaled bf16 tolerance of tests/test_kernels_gpu.py on that file's random-normal data at K = 14336."""
import pytest
import torch

import _exact as E

torch.set_grad_enabled(False)
BF = torch.bfloat16

SCOPES = ("every output", "one ragged tile", "one output row")


def _scope_mask(scope, M, N, tile=64):
    m = torch.zeros(M, N, dtype=torch.bool)
    if scope == "every output":
        m[:] = True
    elif scope == "one ragged tile":
        m[(M - 1) // tile * tile:, (N - 1) // tile * tile:] = True
    else:
        m[M - 1] = True
    return m


def _operands(M, N, K, seed):
    x, w = E.ints((M, K), seed=seed), E.ints((N, K), seed=seed + 7)
    bias, gamma, res = E.epilogue_operands(M, N, seed)
    return x, w, bias, gamma, res


def _run(x, w, bias, gamma, res, kstep, ksplit, mutant=None, relu=False, out_dtype=BF):
    K = w.shape[1]
    xb = E.poisoned(x, pad=16, guard=0) if mutant == "lda gap read as data" else x
    acc = E.model_gemm(xb, w, kstep=kstep, ksplit=ksplit, mutant=mutant, K=K)
    return E.model_epilogue(acc, bias, gamma, res, relu, out_dtype, mutant)


def _honest_cases():
    out = []
    for name, (_, _, shapes) in E.LINEAR_ROUTES.items():
        out += [(name, s, 1) for s in shapes]
    out += [("splitk", (M, N, K), ks) for (M, N, K, ks) in E.SPLITK]
    for (B, H, W, ws, K, N) in E.WINDOWS:                      # the window forms are GEMMs over the padded window-order rows (mode 2: N and K swapped)
        Mw = B * -(-H // ws) * -(-W // ws) * ws * ws
        out += [("window gather", (Mw, N, K), 1), ("window scatter", (Mw, K, N), 1)]
    out += [("bmm", (M, N, K), 1) for (_, M, N, K) in E.BMM] + [("bmm shared_a", E.BMM_SHARED, 1)]
    out += [("gemv", (1, N, K), 1) for N in E.GEMV_N for K in E.GEMV_K]
    out += [("gemv_rows", (B, N, K), 1) for B in E.ROWS_B for N in E.GEMV_Q_N for K in E.ROWS_K]
    out += [("gemv_w8_rows", (B, N, K), 1) for B in E.W8_ROWS_B for N in E.GEMV_Q_N for K in E.GEMV_Q_K]
    out += [("qkv_rope", (1, (H + 2 * Hkv) * D, K), 1) for (H, Hkv, D, K) in E.QKV]
    out += [("linear_rows", s, 1) for s in E.LINEAR_ROWS]
    out += [("f8", s, 1) for s in E.F8]
    return out


@pytest.mark.parametrize("name,shape,ksplit", _honest_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_honest_model_is_exact(name, shape, ksplit):
    """fp32 accumulation of the integer cases is exact in any order: K steps of 32 and 64, the case's K split, scrambled K — all equal float64"""
    M, N, K = shape
    x, w, bias, gamma, res = _operands(M, N, K, seed=M + N + K)
    for out_dtype in (BF, torch.float32):
        r = res.to(out_dtype)
        want = E.reference(x, w, bias, gamma, r, relu=True, out_dtype=out_dtype)
        for kstep in (32, 64):
            got = _run(x, w, bias, gamma, r, kstep, ksplit, relu=True, out_dtype=out_dtype)
            assert torch.equal(got, want), E.explain(got, want, x, w)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    got = _run(x[:, perm], w[:, perm], None, None, None, 64, max(ksplit, 3), out_dtype=torch.float32)
    assert torch.equal(got, E.reference(x, w))


@pytest.mark.parametrize("N", E.GEMV_Q_N)
@pytest.mark.parametrize("K", E.GEMV_Q_K)
def test_honest_model_is_exact_on_scaled_weights(N, K):
    """the fp8 (per-row power-of-two scales) and MXFP4 (per-block scales, one byte-0 block per row) GEMV cases: exact on their unit grid"""
    x = E.ints((1, K), seed=K)
    w = E.ints((N, K), seed=N + K) * torch.ldexp(torch.ones(N), ((torch.arange(N) * 3) % 4 - 2).to(torch.int32))[:, None]
    _, _, deq, _ = E.mxfp4_rows(N, K, seed=N + K)
    for wm, unit in ((w, 0.25), (deq, 1.0)):
        for out_dtype in (BF, torch.float32):
            want = E.reference(x, wm, out_dtype=out_dtype, unit=unit)
            for kstep in (32, 64):
                assert torch.equal(E.model_epilogue(E.model_gemm(x, wm, kstep=kstep), out_dtype=out_dtype), want)


@pytest.mark.parametrize("G,R,K,Hd,No", E.MLP3)
def test_honest_model_is_exact_on_mlp3(G, R, K, Hd, No):
    """three chained layers with ReLU and a bf16 rounding between them: the blocked model equals the guarded float64 reference layer by layer"""
    x = E.ints((R, K), seed=R + K)
    for g in range(G):
        ws = [E.ints((n, k), (-1, 1), seed=10 * g + i) for i, (n, k) in enumerate(((Hd, K), (Hd, Hd), (No, Hd)))]
        bs = [E.ints((n,), (-3, -1, 2, 5), seed=20 * g + i) for i, n in enumerate((Hd, Hd, No))]
        h_ref = h_mod = x
        for i in range(3):
            last = i == 2
            h_ref = E.reference(h_ref, ws[i], bs[i], relu=not last, out_dtype=torch.float32 if last else BF).float()
            h_mod = E.model_epilogue(E.model_gemm(h_mod, ws[i], kstep=16), bs[i], relu=not last, out_dtype=torch.float32 if last else BF).float()
            assert torch.equal(h_mod, h_ref), (g, i)


MUTANT_SHAPES = [(150, 136, 72, 1), (300, 200, 2048, 4), (213, 264, 14336, 8)]        # ragged M and N; short, long and the Llama down-projection K


@pytest.mark.parametrize("scope", SCOPES)
@pytest.mark.parametrize("M,N,K,ksplit", MUTANT_SHAPES)
def test_every_gemm_mutant_fails(M, N, K, ksplit, scope):
    x, w, bias, gamma, res = _operands(M, N, K, seed=K)
    want = E.reference(x, w, bias, gamma, res, out_dtype=BF)
    honest = _run(x, w, bias, gamma, res, 64, ksplit)
    assert torch.equal(honest, want)
    mask = _scope_mask(scope, M, N)
    survived = []
    for mutant in E.GEMM_MUTANTS:
        if "split-K" in mutant and ksplit == 1:
            continue
        mask_m = mask
        bad = _run(x, w, bias, gamma, res, 64, ksplit, mutant=mutant)
        got = torch.where(mask_m, bad, honest)
        wrong = float((got != want)[mask_m].float().mean())
        print(f"M={M} N={N} K={K} ksplit={ksplit} {scope:16s} {mutant:50s} changes {100 * wrong:5.1f} % of the outputs it touches")
        if torch.equal(got, want):
            survived.append(mutant)
        else:
            assert "first (m, n)" in E.explain(got, want, x, w)
    assert not survived, survived


@pytest.mark.parametrize("scope", SCOPES)
@pytest.mark.parametrize("K", [4096, 14336])
def test_every_mxfp4_mutant_fails(K, scope):
    N = 70                                                 # weight rows 64 .. 69: the ragged last 64-row group; row 69: one output
    _, scales, deq, elems = E.mxfp4_rows(N, K, seed=K)
    x = E.ints((1, K), seed=3)
    want = E.reference(x, deq, out_dtype=BF)
    honest = E.model_epilogue(E.model_gemm(x, deq, kstep=32), out_dtype=BF)
    assert torch.equal(honest, want)
    mask = torch.zeros(1, N, dtype=torch.bool)
    mask[0, {"every output": 0, "one ragged tile": 64, "one output row": N - 1}[scope]:] = True
    survived = []
    for mutant in E.MXFP4_MUTANTS:
        wm = E.mxfp4_mutant_weights(elems, scales, mutant)
        assert not torch.equal(wm, deq)
        got = torch.where(mask, E.model_epilogue(E.model_gemm(x, wm, kstep=32), out_dtype=BF), honest)
        if torch.equal(got, want):
            survived.append(mutant)
    assert not survived, survived


def test_mxfp4_rows_mean_what_the_project_dequantises():
    """the host-built codes and scales are the project's format: ops.mxfp4_dequant (plain torch) gives the same matrix, packed rows included"""
    from videoglamm_amd import ops
    codes, scales, deq, _ = E.mxfp4_rows(5, 4096, seed=1)
    live = (scales != 0).repeat_interleave(32, dim=1)          # (a byte-0 block: 2^-127 to mxfp4_dequant, nothing to the kernel and to the reference here)
    assert int((~live).sum()) == 5 * 32 and bool((deq[~live] == 0).all())
    assert torch.equal(ops.mxfp4_dequant(codes, scales)[live], deq[live])
    assert torch.equal(ops.mxfp4_dequant(ops.mxfp4_pack(codes, scales))[live], deq[live])
    assert torch.equal(E.e4m3_codes(E.ints((4, 16))).view(torch.float8_e4m3fn).float(), E.ints((4, 16)))


def test_mutant_list_is_complete():
    table = {
        "last K element dropped", "last 8 K elements dropped", "one K step dropped", "one K step counted twice",
        "split-K boundary element counted by both slices", "a split-K slice dropped", "x chunk i paired with w chunk i + 1",
        "an output tile shifted by one row", "bias missing in the last partial column group", "lda gap read as data",
        "one MXFP4 block with its neighbour's scale", "packed MXFP4: the scale of block 64 u + lane taken from u + 1",
    }
    assert set(E.MUTANTS) == table and len(E.MUTANTS) == 12
    src = open(E.__file__).read()
    for name in E.GEMM_MUTANTS:                              # every name is implemented by the model, not only listed
        assert src.count('"%s"' % name) >= 2, name


def test_guard_refuses_inexact_cases():
    x, w = E.ints((2, 64)) * 2.0 ** 12, E.ints((3, 64), seed=1) * 2.0 ** 12
    with pytest.raises(AssertionError):
        E.reference(x, w)
    with pytest.raises(AssertionError):
        E.reference(E.ints((2, 64)), E.ints((3, 64), seed=1), bias=torch.full((3,), 0.3))


def test_poison_and_sentinel_show():
    x = E.ints((5, 24))
    big = E.poisoned(x, dtype=BF)
    assert torch.equal(big[:5, :24].float(), x) and float(big[:5, 24:].float().abs().min()) >= E.POISON and float(big[5:].float().abs().min()) >= E.POISON
    buf, view = E.sentinel_out(5, 33, BF, "cpu")
    view.copy_(E.ints((5, 33)).to(BF))
    assert E.sentinel_intact(buf, 5, 33)
    buf[0, 3] = 1.0
    assert not E.sentinel_intact(buf, 5, 33)


def test_explain_names_the_lost_product():
    x, w = E.ints((70, 128), seed=1), E.ints((130, 128), seed=2)
    want = E.reference(x, w)
    got = want.clone()
    got[65, 129] -= float(x[65, 127] * w[129, 127])
    s = E.explain(got, want, x, w)
    assert "(65, 129)" in s and "removed" in s and "tile 64: (1, 2) + (1, 1)" in s and "127" in s


def test_tolerance_gap_is_recorded():
    """The gap the exact tests close.  On test_gemm_splitk / test_decode_gemv's data (x ~ N(0, 1), w ~ N(0, 1) K^-0.5, bf16, K = 14336) a result
    that loses one K element, eight K elements or a whole 64-element K step IN EVERY OUTPUT passes tol(bf16, K) (atol 0.3 on outputs of size 1);
    each fails the rtol = atol = 2e-2 those tests use after this change, and each fails the exact comparison on integer data."""
    M, N, K = 16, 256, 14336
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g).to(BF).float()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF).float()
    want = (x.double() @ w.double().t()).float().to(BF).float()
    xi, wi = E.ints((M, K), seed=1), E.ints((N, K), seed=2)
    want_i = E.reference(xi, wi, out_dtype=BF)
    loose = dict(rtol=2e-2, atol=2e-2 * (K / 64) ** 0.5)          # tol(torch.bfloat16, K) of tests/test_kernels_gpu.py
    tight = dict(rtol=2e-2, atol=2e-2)

    def passes(a, b, **t):
        try:
            torch.testing.assert_close(a, b, **t)
            return True
        except AssertionError:
            return False

    for mutant in ("last K element dropped", "last 8 K elements dropped", "one K step dropped"):
        got = E.model_gemm(x, w, kstep=64, mutant=mutant).to(BF).float()
        got_i = E.model_gemm(xi, wi, kstep=64, mutant=mutant).to(BF)
        p_loose, p_tight, changed = passes(got, want, **loose), passes(got, want, **tight), float((got_i != want_i).float().mean())
        print(f"K = {K}: '{mutant}' in every output: max abs err {float((got - want).abs().max()):.3f}; passes tol(bf16, K) (atol {loose['atol']:.2f}): {p_loose}; "
              f"passes rtol = atol = 2e-2: {p_tight}; exact integer test: {100 * changed:.0f} % of the outputs differ")
        assert p_loose, "the old tolerance was expected to let this mutant through"
        assert not p_tight
        assert changed > 0.5
    honest = E.model_gemm(x, w, kstep=64).to(BF).float()
    assert passes(honest, want, **tight)
