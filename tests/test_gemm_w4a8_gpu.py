"""vg_gemm_w4a8 / ops.linear_w4a8: e4m3 activations x packed MXFP4 weight rows (the prefill GEMM of cfg prefill_gemm = "mxfp4").

  1  exact (torch.equal): host-built e4m3 codes with power-of-two row scales against E.mxfp4_rows packed by ops.mxfp4_pack; E.reference proves the
     exactness of every case itself.  Four shapes (ragged M and N tiles, N < 128, M = 17, every SPL) x {bf16, fp32} x {plain, residual}, and once
     per shape and dtype with strided, poisoned operands into a sentinel-guarded output.
  2  a weight row whose every scale byte is 0 under non-zero codes gives exactly 0.0 (the hardware's own reading, 2^-127, is not zero)
  3  GLU == ops.swiglu of the same kernel's bf16 output over the 2N rows, bit for bit
  4  rows 0..16 of an M = 130 call == the M = 17 call on those rows
  5  random data through the real quantisers against the float64 product of the dequantised operands
  6  refusals (nothing is launched)"""
import pytest
import torch

import _exact as E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(130, 264, 3072), (33, 136, 4096), (200, 72, 8192), (17, 40, 14336)]
A_EXPS = (-2, -1, 0, 1)           # activation row scales; the weights' block scales are >= 1: every product is a multiple of 2^-2
UNIT = 2.0 ** -2
_CACHE = {}


def _exact_case(M, N, K):
    """host operands of one exact case, built once per shape: x [M,K] integers, row scales, codes, MXFP4 rows and what they mean"""
    key = (M, N, K)
    if key not in _CACHE:
        from videoglamm_amd import ops
        x = E.ints((M, K), seed=M + K)
        qs = E.pow2(M, A_EXPS, seed=1)
        codes, scales, w_mean, _ = E.mxfp4_rows(N, K, seed=N)
        packed = ops.mxfp4_pack(codes, scales)
        _CACHE[key] = (x, qs, x * qs[:, None], packed, w_mean)
    return _CACHE[key]


def _strided_w(packed, K):
    """the packed rows inside a buffer whose rows are 32 bytes longer (gap = 0x77 code bytes) with two guard rows whose heads hold 0xFE"""
    from videoglamm_amd import ops
    N, rl = packed.shape
    big = torch.full((N + 2, rl + 32), 0x77, dtype=torch.uint8)
    big[:N, :rl] = packed
    big[N:, : 64 * ops.MXFP4_K[K]] = 0xFE
    return big


@pytest.mark.parametrize("out_dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact(cuda, out_dt, M, N, K):
    from videoglamm_amd import ops
    x, qs, xs, packed, w_mean = _exact_case(M, N, K)
    q = E.e4m3_codes(x).to(cuda)
    pk = packed.to(cuda)
    res = E.ints((M, N), (-8, -3, 1, 6), seed=3).to(out_dt)
    for r in (None, res):
        want = E.reference(xs, w_mean, residual=r, out_dtype=out_dt, unit=UNIT)
        got = ops.linear_w4a8(q, qs.to(cuda), pk, residual=None if r is None else r.to(cuda), out_dtype=out_dt)
        E.check(got, want, xs, w_mean, f"linear_w4a8 M={M} N={N} K={K} residual={r is not None}")
    # strided, poisoned operands into a sentinel-guarded destination
    qb = E.e4m3_codes(E.poisoned(x, poison=224.0)).to(cuda)
    wb = _strided_w(packed, K).to(cuda)
    rb = E.poisoned(res.float(), pad=8, dtype=out_dt).to(cuda)
    big, view = E.sentinel_out(M, N, out_dt, cuda)
    want = E.reference(xs, w_mean, residual=res, out_dtype=out_dt, unit=UNIT)
    got = ops.linear_w4a8(qb[:M, :K], qs.to(cuda), wb[:N, : packed.shape[1]], residual=rb[:M, :N], out_dtype=out_dt, out=view)
    assert got.data_ptr() == view.data_ptr()
    E.check(view, want, xs, w_mean, f"linear_w4a8 strided + poisoned M={M} N={N} K={K}")
    assert E.sentinel_intact(big, M, N), "written outside [M, N]"


@pytest.mark.parametrize("M,N,K", [(33, 136, 4096), (17, 40, 14336)])
def test_all_zero_scale_row_is_exactly_zero(cuda, M, N, K):
    from videoglamm_amd import ops
    x = E.ints((M, K), seed=5)
    codes, scales, _, elems = E.mxfp4_rows(N, K, seed=9)
    rows = [3, N - 1]
    scales[rows] = 0                         # every block of these rows: scale byte 0 under non-zero codes
    assert bool((codes[rows] != 0).all())
    w_mean = E.mxfp4_mean(elems, scales)
    qs = torch.ones(M)
    want = E.reference(x, w_mean, out_dtype=F32)
    got = ops.linear_w4a8(E.e4m3_codes(x).to(cuda), qs.to(cuda), ops.mxfp4_pack(codes, scales).to(cuda), out_dtype=F32)
    g = got.cpu()
    assert bool((g[:, rows] == 0.0).all()), f"a zero-scale row is not zero: max |y| = {float(g[:, rows].abs().max())!r}"
    E.check(got, want, x, w_mean, "zero-scale rows")


def _random_case(cuda, M, rows, K, seed):
    from videoglamm_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(rows, K, generator=g) * 0.02).to(BF)
    q, qs = ops.quantize_fp8(x.to(cuda))
    codes, scales = ops.quantize_mxfp4_rows(w)
    packed = ops.mxfp4_pack(codes, scales).to(cuda)
    xd = q.cpu().view(torch.float8_e4m3fn).double() * qs.cpu().double()[:, None]
    wd = ops.mxfp4_dequant(codes, scales).double()
    return q, qs, packed, xd @ wd.t()


@pytest.mark.parametrize("M,F_,K", [(130, 136, 3072), (33, 72, 4096), (200, 264, 8192), (17, 40, 14336)])
def test_glu_equals_swiglu_of_linear(cuda, M, F_, K):
    from videoglamm_amd import ops
    q, qs, packed, _ = _random_case(cuda, M, 2 * F_, K, seed=F_)
    lin = ops.linear_w4a8(q, qs, packed, out_dtype=BF)
    assert lin.shape == (M, 2 * F_)
    want = ops.swiglu(lin)
    got = ops.linear_w4a8(q, qs, packed, glu=True, out_dtype=BF)
    assert got.shape == (M, F_) and bool(got.float().abs().sum() > 0)
    assert torch.equal(got, want), f"GLU != swiglu(linear): {int((got != want).sum())} of {got.numel()} differ"


def test_rows_independent(cuda):
    from videoglamm_amd import ops
    M, N, K = SHAPES[0]
    x, qs, _, packed, _ = _exact_case(M, N, K)
    q, qsd, pk = E.e4m3_codes(x).to(cuda), qs.to(cuda), packed.to(cuda)
    for dt in (BF, F32):
        full = ops.linear_w4a8(q, qsd, pk, out_dtype=dt)
        head = ops.linear_w4a8(q[:17].contiguous(), qsd[:17].contiguous(), pk, out_dtype=dt)
        assert torch.equal(full[:17], head)


def _check_random(got32, got16, want64, what):
    """fp32 output: test_gemm_f8's rtol = atol = 1e-3 (the same accumulation structure).  bf16 output: within one bf16 ulp of the float64 value's rounding.
    Where |value| < 2^-3 a bf16 ulp (< 2^-10) is smaller than the 1e-3 the fp32 comparison grants the accumulation itself (sums that cancel to nearly
    zero), so there the ulp of 2^-3 stands in.  And the bf16 output must be the rounding of the same launch's fp32 output bit for bit: the two
    instantiations differ in the last store only."""
    w32 = want64.float()
    print(f"{what}: fp32 max abs err {float((got32.cpu().double() - want64).abs().max()):.3e}, max |want| {float(want64.abs().max()):.3e}")
    torch.testing.assert_close(got32.cpu(), w32, rtol=1e-3, atol=1e-3)
    assert torch.equal(got16, got32.to(BF)), f"{what}: the bf16 output is not the rounding of the fp32 output"
    wb = w32.to(BF).double()
    ulp = torch.exp2(torch.floor(torch.log2(wb.abs().clamp_min(2.0 ** -3))) - 7)
    d = (got16.cpu().double() - wb).abs() / ulp
    print(f"{what}: bf16 max distance {float(d.max()):.3f} ulp")
    assert float(d.max()) <= 1.0, f"{what}: bf16 output {float(d.max())} ulp from the rounded float64 value"


def test_random_glu(cuda):
    """(300, 512, 4096), GLU.  The fp32 GLU output is compared with silu(gate) * up of the float64 products (rtol = atol = 1e-3); the bf16 contract rounds gate,
    up and silu(gate) to bf16 before the product, so there the one-ulp comparison is made on the bf16 gate | up output the GLU is defined on, and the bf16
    GLU output must equal ops.swiglu of it bit for bit."""
    from videoglamm_amd import ops
    M, F_, K = 300, 512, 4096
    q, qs, packed, want = _random_case(cuda, M, 2 * F_, K, seed=11)
    lin32 = ops.linear_w4a8(q, qs, packed, out_dtype=F32)
    lin16 = ops.linear_w4a8(q, qs, packed, out_dtype=BF)
    _check_random(lin32, lin16, want, "gate|up")
    g, u = want[:, :F_], want[:, F_:]
    glu64 = g * torch.sigmoid(g) * u
    glu32 = ops.linear_w4a8(q, qs, packed, glu=True, out_dtype=F32)
    print(f"glu: fp32 max abs err {float((glu32.cpu().double() - glu64).abs().max()):.3e}")
    torch.testing.assert_close(glu32.cpu(), glu64.float(), rtol=1e-3, atol=1e-3)
    assert torch.equal(ops.linear_w4a8(q, qs, packed, glu=True, out_dtype=BF), ops.swiglu(lin16))


def test_random_residual(cuda):
    from videoglamm_amd import ops
    M, N, K = 300, 256, 14336
    q, qs, packed, want = _random_case(cuda, M, N, K, seed=12)
    r = torch.randn(M, N, generator=torch.Generator().manual_seed(13)).to(BF)
    want = want + r.double()
    got32 = ops.linear_w4a8(q, qs, packed, residual=r.float().to(cuda), out_dtype=F32)
    got16 = ops.linear_w4a8(q, qs, packed, residual=r.to(cuda), out_dtype=BF)
    _check_random(got32, got16, want, "down + residual")


def test_refusals(cuda):
    import ctypes
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    assert not ops.linear_w4a8_supported(264, 2048) and not ops.linear_w4a8_supported(260, 4096)
    assert all(ops.linear_w4a8_supported(264, K) for K in (3072, 4096, 8192, 14336))

    def call(M, N, K, ldw=None, rowlen=None):
        rl = rowlen or (64 * ops.MXFP4_K.get(K, 2) + K // 2)
        ldw = ldw or rl
        q = torch.zeros(M, K, dtype=torch.uint8, device=cuda)
        qs = torch.ones(M, device=cuda)
        w = torch.zeros(N * ldw + 64, dtype=torch.uint8, device=cuda)
        y = torch.full((M, N), E.SENTINEL, dtype=BF, device=cuda)
        rc = lib.vg_gemm_w4a8(q.data_ptr(), K, qs.data_ptr(), w.data_ptr(), ldw, y.data_ptr(), N, None, 0, M, N, K, 1, 0,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool((y == E.SENTINEL).all()), "a refused call wrote its output"
        return rc

    assert call(64, 264, 2048) == -3                      # VG_ERR_UNSUPPORTED: no packed row of that length
    assert call(16, 264, 4096) != 0                       # M = 16: the decode GEMVs' range
    assert call(64, 260, 4096) == -3                      # N not a multiple of 8
    assert call(64, 264, 4096, ldw=128 + 2048 + 8) == -1  # VG_ERR_ARG: row stride not a multiple of 16
    with pytest.raises(_lib.VGKernelError):
        ops.linear_w4a8(torch.zeros(16, 4096, dtype=torch.uint8, device=cuda), torch.ones(16, device=cuda),
                        torch.zeros(264, 128 + 2048, dtype=torch.uint8, device=cuda))
