"""Norms, norm prologues, activations and rotations against float64 at rounding level (-m gpu).

Everything that is not a contraction or a softmax used to be checked at rtol = atol = 2e-2 in bf16 only (test_kernels_gpu.tol): LayerNorm / RMSNorm,
the norm prologues fused into GEMVs and GEMMs, the activation functions and the rotations.  Here (tests/_rowwise_ref.py, which derives every
bound) each kernel output is compared with the float64 statement on the stored operands:
  * element check: |got - ref64| <= 1/2 ulp_out(ref64) + slack, slack a closed form of the fp32 arithmetic times a multiple measured from the
    CPU fp32 statement (x 4, floor 4), never from a kernel;
  * share check (bf16 outputs): the share of elements that differ from ref64 rounded once is at most max(4 x the CPU statement's share, 1e-3);
  * torch.equal where the arithmetic is fully specified: bf16 rope_half_ and the rotation of rope_kv_append_, cast, mask_for_mem(binarize = 1), ReLU.
Inputs: random rows N(3, 1) plus probe rows (spikes on the edges of the per-lane chunk walk of the route the case is meant for, offset, step,
quiet and constant rows); activations on a grid over [-12, 12] plus +-0, +-20, +-88, +-100 and the largest finite bf16.

tests/test_rowwise_accuracy_selfcheck.py proves on the CPU that honest fp32 models (torch's statements, a transcription of norm_short_kernel's
lane-strided sums, a transcription of vg_gelu_erf) pass and that each of these wrong kernels fails, in every shape class it applies to:
   1 last column dropped from the statistics          10 LayerNorm that forgets b on the last chunk
   2 last 8-column chunk dropped                      11 tanh GELU where the erf GELU is specified
   3 one column counted twice                         12 quick-GELU with 1.7 for 1.702
   4 divisor C - 1                                    13 SwiGLU without the bf16 rounding of the gate
   5 divisor padded to the lane width                 14 SwiGLU with gate and up swapped
   6 one-pass fp32 variance                           15 rope_half with fp32 products
   7 eps x 10                                         16 rope_half with the sign of sin flipped on one half
   8 RMSNorm without the intermediate rounding        17 axial RoPE reading the table row of tok instead of tok % n_grid
   9 RMSNorm that subtracts a mean

Routes: the library has no query for the route launch_norm_t takes, so _norm_route() restates its rule (vg_rowops.hip) and every case asserts the
route it is meant for; the GEMM epilogue cases assert vg_gemm_route.

Measured on the MI355X (also DESIGN.md section 2): all cases pass, no kernel was found wrong.  Per route, over its cases: the largest slack
multiple the kernel needed | the CPU fp32 statement needed | the largest allowed (4 x, floor 4); the largest mismatch share kernel | statement.
  layernorm  workgroup scalar / register / streaming      2.24 / 1.82 / 0.69 | 2.59 / 2.29 / 2.58 | 10.4 / 9.1 / 10.3     1.3e-4 / 3.3e-4 / 1.0e-4 | 1.7e-4 / 2.1e-4 / 1.7e-4
  layernorm  16 lanes / wave register / wave scalar       2.54 / 2.49 / 2.01 | 2.83 / 3.12 / 2.71 | 11.3 / 12.5 / 10.8    1.1e-4 / 1.7e-4 / 0.9e-4 | 1.5e-4 / 1.9e-4 / 1.1e-4
  layernorm  norm_short <64,2> <64,3> <64,6> <64,8>       0.32 / 1.15 / 1.33 / 1.10 | 2.53 .. 3.54 | 10.1 .. 14.2         0.3e-4 .. 1.4e-4 | 0.7e-4 .. 1.2e-4
  layernorm  norm_short <8,3> <8,5> <8,9> <16,9>          0.45 / 0.42 / 0.82 / 0.85 | 3.06 .. 3.70 | 12.2 .. 14.8         0.7e-4 .. 1.3e-4 | 1.2e-4 .. 2.0e-4
  rmsnorm    workgroup / 16 lanes / wave routes           0.86 / 1.36 / 1.59 | 1.19 / 1.48 / 1.70 | 4.7 / 5.9 / 6.8       <= 2.6e-5 | <= 2.3e-5
  (norm_kernel's own second grid-stride pass: 8197 x 2048 bf16 wave register 0.52 | 2.48 | 9.9; 32773 x 256 fp32 16 lanes 2.29 | 3.32 | 13.3)
  rmsnorm    the eight norm_short instantiations          <= 0.36 | 0.00 | 4.0                                            <= 1.2e-5 | <= 1.2e-5
  prologues  13 decode projection cases, decode_qkv_rope  bf16 0.00, fp32 1.15 | 1.12 | 4.0 / 4.5                         0 | 0
  prologues  linear_rows / linear_ln / window / mlp_rows  0.00 / 0.32 / 0.37 / 0.00 | 1.51 / 2.24 / 2.05 / - | 6.0 / 9.0 / 8.2 / 2     0 / 1.1e-4 / 0.5e-4 / 0 | 2.5e-4 / 1.5e-4 / 1.0e-4 / 0
  erf GELU   act_kernel and every vg_gemm route           2.44 | 3.16 | 12.7                                              0 | 0  (x >= -1)
  quick-GELU / SiLU / sigmoid, the same                   2.08 / 2.00 / 1.50 | 1.71 / 1.40 / 1.48 | 6.8 / 5.6 / 5.9       0.4e-4 / 5.0e-4 / 2.1e-4 | 2.1e-4 / 0 / 0
  swiglu, the GLU epilogues (skinny, glds, p8; each shape holds the gate grid)  1.12 | 0.96 | 4.0                         2.0e-4 | 0
  mask_for_mem (sigmoid mode)                             1.74 | 2.34 | 9.4                                               0 | 0.4e-4
  rope_axial scalar / vec / heads, rope_half fp32, rope_kv_append fp32, axpby      0.77 / 0 / 0, 0.90, 0.81, 0.62 of the fixed multiple 2
  torch.equal: bf16 rope_half_, bf16 rope_kv_append_ (both kernels, pos0 and pos_dev), cast, mask_for_mem(binarize), ReLU, the sentinel outputs.
(SiLU's and sigmoid's shares are two or three of the 5000 bf16 grid points: v_exp_f32 / v_rcp_f32 against torch's libm.)
Findings: none about a kernel.  About ref64's model of the roundings (corrected in tests/_rowwise_ref.py on the CPU, every wrong kernel still fails):
an intermediate bf16 rounding next to a tie is ambiguous for an honest fp32 kernel; rows built to cancel and repeated values of a weightless row
distort the share; torch's own fp32 GELU overflows at the largest finite bf16 where vg_gelu_erf does not.
"""
import os
import subprocess
import sys

import pytest
import torch

import _exact as E
import _rowwise_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BF, F32 = R.BF, R.F32
LN_EPS, RMS_EPS = 1e-6, 1e-5


def _d(t, cuda):
    return None if t is None else t.to(cuda)


# ------------------------------------------------------------------ A. ops.layernorm / ops.rmsnorm
_SHORT_1024 = {1408: (64, 3), 1024: (64, 2), 4096: (64, 8), 3072: (64, 6)}
_SHORT_4096 = {576: (8, 9), 1152: (16, 9), 288: (8, 5), 144: (8, 3)}


def _norm_route(rows, C, dt, odt, aligned=True):
    """(route, TPR, NV) of launch_norm_t (vg_rowops.hip), restated: `aligned` = row strides multiples of NV and 16-byte aligned pointers"""
    nv = 8 if dt == BF else 4
    vec = C % nv == 0 and aligned
    if dt == BF and odt == BF and vec:
        if rows >= 1024 and C in _SHORT_1024:
            return "norm_short<%d,%d>" % _SHORT_1024[C], _SHORT_1024[C][0], nv
        if rows >= 4096 and C in _SHORT_4096:
            return "norm_short<%d,%d>" % _SHORT_4096[C], _SHORT_4096[C][0], nv
    if rows < 1024 or (vec and C > 64 * nv * 4):
        if not vec:
            return "workgroup scalar", 256, 1
        return ("workgroup register" if C <= 256 * nv * 4 else "workgroup streaming"), 256, nv
    if vec and C <= 16 * nv * 4:
        return "16 lanes register", 16, nv
    return ("wave register", 64, nv) if vec else ("wave scalar", 64, 1)


def _second_pass_rows(route, tpr):
    """rows the capped grid of a norm_short instantiation covers in one pass (launch_norm_short: 256 x 8 workgroups, 256 x 4 from nine chunks per lane)"""
    nj = int(route.split(",")[1].rstrip(">"))
    return 256 * (4 if nj >= 9 else 8) * (256 // tpr)


NORMS = [  # rows, C, input dtype, output dtype, route meant
    (5, 4, BF, BF, "workgroup scalar"), (5, 1404, BF, BF, "workgroup scalar"), (5, 1404, BF, F32, "workgroup scalar"),
    (3, 4096, BF, BF, "workgroup register"), (3, 4096, BF, F32, "workgroup register"), (3, 2048, F32, F32, "workgroup register"),
    (3, 2048, F32, BF, "workgroup register"), (3, 8200, BF, BF, "workgroup streaming"),
    (1027, 144, BF, BF, "16 lanes register"), (1027, 288, BF, BF, "16 lanes register"), (1027, 288, BF, F32, "16 lanes register"),
    (1027, 512, BF, BF, "16 lanes register"), (1027, 256, F32, F32, "16 lanes register"),
    (1027, 520, BF, BF, "wave register"), (1027, 520, BF, F32, "wave register"), (1027, 2048, BF, BF, "wave register"),
    (1027, 260, F32, F32, "wave register"), (1027, 260, F32, BF, "wave register"), (1027, 1024, F32, F32, "wave register"),
    (1027, 516, BF, BF, "wave scalar"), (1027, 258, F32, F32, "wave scalar"),
    (1027, 1408, BF, BF, "norm_short<64,3>"), (1027, 1024, BF, BF, "norm_short<64,2>"), (1027, 4096, BF, BF, "norm_short<64,8>"),
    (1027, 3072, BF, BF, "norm_short<64,6>"), (4101, 576, BF, BF, "norm_short<8,9>"), (4101, 1152, BF, BF, "norm_short<16,9>"),
    (4101, 288, BF, BF, "norm_short<8,5>"), (4101, 144, BF, BF, "norm_short<8,3>"),
    # one row count just past what the capped grid covers in one pass, once per (TPR, NJ) class: the probe rows are the last rows, which the second
    # grid-stride pass and its clamped prefetch produce
    (8192 + 5, 1408, BF, BF, "norm_short<64,3>"), (8192 + 5, 4096, BF, BF, "norm_short<64,8>"),
    (16384 + 5, 1152, BF, BF, "norm_short<16,9>"), (32768 + 33, 576, BF, BF, "norm_short<8,9>"), (65536 + 33, 144, BF, BF, "norm_short<8,3>"),
    # the same for norm_kernel's register-resident path, which is grid-stride too (2048 workgroups of 4 rows / of 16 rows)
    (8192 + 5, 2048, BF, BF, "wave register"), (32768 + 5, 256, F32, F32, "16 lanes register"),
]
_NAME = {BF: "bf16", F32: "fp32"}


def _checked_rows(rows):
    """the rows the CPU compares: all, or (tall cases) the first 128 and the last 389 — every row of the second pass and the clamped prefetch, and
    the full groups before them"""
    if rows <= 4200:
        return torch.arange(rows)
    return torch.cat([torch.arange(128), torch.arange(rows - 389, rows)])


def _norm_cases(rows, C, dt, odt, rms, tpr, nv, has_w, route, run):
    """run(x on the CPU, w, b, eps) -> the kernel's output [rows, C]; -> the case over all rounds and the outputs on the checked rows.
    The selection rule of the inputs: the rows are drawn from seed 2, or from the first of the seeds 3, 4, 5 with which the CPU fp32 statement meets
    the helper's precondition (its own mismatch share <= 2.5e-4) — decided on the CPU before the kernel runs; a few-row case without weights counts
    a few thousand distinct values, where three statement roundings already exceed it.  No seed of the four: the case fails."""
    w, b = R.norm_weights(C)
    w, b = (w, b) if has_w else (None, None)
    b = None if rms else b
    eps = RMS_EPS if rms else LN_EPS
    idx = _checked_rows(rows)
    name = f"{'rmsnorm' if rms else 'layernorm'} {rows}x{C} {_NAME[dt]}->{_NAME[odt]} w={int(has_w)}"
    for seed in (2, 3, 4, 5):
        rounds = R.build_norm_rounds(rows, C, dt, rms, tpr, nv, seed=seed)
        cases = [R.norm_case(name, x[idx], w, b, eps, rms, odt, route=route, probes={int((idx == r).nonzero()[0]): k for r, k in probes.items()})
                 for x, probes in rounds]
        whole = R.cat_cases(name, cases)
        if odt != BF or whole.shares(whole.model())[1] <= R.SHARE_CPU_MAX:
            break
    gots = []
    for x, _ in rounds:
        got = run(x, w, b, eps)
        assert got.shape == x.shape and got.dtype == odt
        gots.append(got.cpu()[idx].reshape(-1))
    return whole, torch.cat(gots)


@pytest.mark.parametrize("has_w", [True, False], ids=["w", "now"])
@pytest.mark.parametrize("cfg", NORMS, ids=lambda c: f"{c[0]}x{c[1]}-{_NAME[c[2]]}-{_NAME[c[3]]}")
def test_norms(cuda, cfg, has_w):
    """every route of launch_norm_t, LayerNorm and RMSNorm, with w / b present and None"""
    from videoglamm_amd import ops
    rows, C, dt, odt, meant = cfg
    route, tpr, nv = _norm_route(rows, C, dt, odt)
    assert route == meant, (route, meant)
    if route.startswith("norm_short") and rows > 8000:
        assert _second_pass_rows(route, tpr) < rows <= _second_pass_rows(route, tpr) + 64, "not a second-pass case"
    if route in ("wave register", "16 lanes register") and rows > 8000:          # launch_norm_t: pgrid = 256 x 8 workgroups of 256 / TPR rows
        assert 2048 * (256 // tpr) < rows <= 2048 * (256 // tpr) + 64, "not a second-pass case"
    for rms in (False, True):
        def run(x, w, b, eps):
            if rms:
                return ops.rmsnorm(x.to(cuda), _d(w, cuda), eps, out_dtype=odt)
            return ops.layernorm(x.to(cuda), _d(w, cuda), _d(b, cuda), eps, out_dtype=odt)
        case, got = _norm_cases(rows, C, dt, odt, rms, tpr, nv, has_w, route, run)
        R.check(case, got)


@pytest.mark.parametrize("rows,C,dt", [(1027, 520, BF), (1027, 144, BF), (1027, 260, F32), (3, 4096, BF)], ids=lambda v: str(v))
def test_norms_fused_qkv_slice(cuda, rows, C, dt):
    """the q / k slice of a fused [rows, 3 C] projection (InternVideo2's QK-RMSNorm): a strided view, 16-byte aligned, so the route of the width holds"""
    from videoglamm_amd import ops
    route, tpr, nv = _norm_route(rows, C, dt, dt, aligned=(C * (2 if dt == BF else 4)) % 16 == 0)
    assert route in ("wave register", "16 lanes register", "workgroup register")
    for rms in (True, False):
        def run(x, w, b, eps):
            g = torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(9)).to(dt).to(cuda)
            g[:, C:2 * C] = x.to(cuda)
            v = g[:, C:2 * C]
            assert not v.is_contiguous()
            return ops.rmsnorm(v, _d(w, cuda), eps) if rms else ops.layernorm(v, _d(w, cuda), _d(b, cuda), eps)
        case, got = _norm_cases(rows, C, dt, dt, rms, tpr, nv, True, route + " (3C view)", run)
        R.check(case, got)


SENTINEL_NORMS = [(5, 1404, BF), (3, 4096, BF), (3, 8200, BF), (1027, 144, BF), (1027, 520, BF), (1027, 516, BF), (1027, 260, F32), (1027, 1408, BF),
                  (4101, 576, BF)]


@pytest.mark.parametrize("rows,C,dt", SENTINEL_NORMS, ids=lambda v: str(v))
def test_norms_sentinel_output(cuda, rows, C, dt):
    """one case per route into a sentinel-filled buffer with guard rows and columns (a row stride of C + 16): equal to the contiguous call bit for
    bit (which test_norms checks against float64), and nothing outside [rows, C] written"""
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    route, tpr, nv = _norm_route(rows, C, dt, dt)
    w, b = R.norm_weights(C)
    x = R.build_norm_rounds(rows, C, dt, False, tpr, nv, seed=3)[0][0].to(cuda)
    wd, bd = w.to(cuda), b.to(cuda)
    for rms in (False, True):
        big, view = E.sentinel_out(rows, C, dt, cuda)
        code = ops.BF16 if dt == BF else ops.F32
        if rms:
            rc = lib.vg_rmsnorm(ops._p(x), C, ops._p(wd), ops._p(view), view.stride(0), rows, C, RMS_EPS, code, code, ops._stream())
            want = ops.rmsnorm(x, wd, RMS_EPS)
        else:
            rc = lib.vg_layernorm(ops._p(x), C, ops._p(wd), ops._p(bd), ops._p(view), view.stride(0), rows, C, LN_EPS, code, code, ops._stream())
            want = ops.layernorm(x, wd, bd, LN_EPS)
        _lib.check(rc, "norm into a strided view")
        print(f"ACC norm sentinel {rows}x{C} {_NAME[dt]} rms={int(rms)} route {route}")
        assert torch.equal(view, want), (route, rms)
        assert E.sentinel_intact(big, rows, C), (route, rms, "written outside [rows, C]")


# ------------------------------------------------------------------ B. norm prologues, isolated by one-hot weights
def _pi(K, tpr, nv, N):
    """N distinct columns: the first and last, both sides of every staging-chunk edge (spike_columns and their neighbours), the rest evenly spread"""
    cols = []
    for c in R.spike_columns(K, tpr, nv):
        cols += [c - 1, c, c + 1]
    cols = [c for c in dict.fromkeys(cols) if 0 <= c < K]
    rest = [c for c in torch.linspace(0, K - 1, N).long().tolist() if c not in set(cols)]
    return torch.tensor((cols + rest)[:N])


def _onehot(N, K, pi, dtype=BF):
    w = torch.zeros(N, K, dtype=dtype)
    w[torch.arange(N), pi] = 1.0
    return w


def _w4_onehot(N, K, pi):
    """packed MXFP4 rows of the one-hot matrix: e2m1 code 2 (= 1.0) at (n, pi[n]), every block scale 2^0 (byte 127)"""
    from videoglamm_amd import ops
    codes = torch.zeros(N, K // 2, dtype=torch.uint8)
    codes[torch.arange(N), pi // 2] = torch.where(pi % 2 == 0, 2, 2 << 4).to(torch.uint8)
    scales = torch.full((N, K // 32), 127, dtype=torch.uint8)
    assert torch.equal(ops.mxfp4_dequant(codes, scales), _onehot(N, K, pi, F32))
    return ops.mxfp4_pack(codes, scales)


def _projections():
    """name -> (rows variant?, input dtype, K, call(ops, x, w on the device, norm_w, eps), weight builder(N, K, pi))"""
    from videoglamm_amd import ops
    plain = lambda N, K, pi: (_onehot(N, K, pi),)                                                        # noqa: E731
    f32w = lambda N, K, pi: (_onehot(N, K, pi, F32),)                                                    # noqa: E731
    w8 = lambda N, K, pi: (E.e4m3_codes(_onehot(N, K, pi, F32)), torch.ones(N))                          # noqa: E731
    w4 = lambda N, K, pi: (_w4_onehot(N, K, pi),)                                                        # noqa: E731
    return {
        "decode_gemv bf16 K=64": (False, BF, 64, lambda x, w, nw, e: ops.decode_gemv(x, *w, norm_w=nw, eps=e), plain),
        "decode_gemv bf16": (False, BF, 3072, lambda x, w, nw, e: ops.decode_gemv(x, *w, norm_w=nw, eps=e), plain),
        "decode_gemv fp32": (False, F32, 3072, lambda x, w, nw, e: ops.decode_gemv(x, *w, norm_w=nw, eps=e), f32w),
        "decode_gemv_p13": (False, BF, 4096, None, plain),
        "decode_gemv_w8": (False, BF, 3072, lambda x, w, nw, e: ops.decode_gemv_w8(x, *w, norm_w=nw, eps=e), w8),
        "decode_gemv_w4": (False, BF, 3072, lambda x, w, nw, e: ops.decode_gemv_w4(x, *w, norm_w=nw, eps=e), w4),
        "decode_gemv_rows K=2048": (True, BF, 2048, lambda x, w, nw, e: ops.decode_gemv_rows(x, *w, norm_w=nw, eps=e), plain),
        "decode_gemv_rows": (True, BF, 3072, lambda x, w, nw, e: ops.decode_gemv_rows(x, *w, norm_w=nw, eps=e), plain),
        "decode_gemm_rows": (True, BF, 3072, lambda x, w, nw, e: ops.decode_gemm_rows(x, *w, norm_w=nw, eps=e), plain),
        "decode_gemm_w8_rows": (True, BF, 3072, lambda x, w, nw, e: ops.decode_gemm_w8_rows(x, *w, norm_w=nw, eps=e), w8),
        "decode_gemm_w4_rows": (True, BF, 3072, lambda x, w, nw, e: ops.decode_gemm_w4_rows(x, *w, norm_w=nw, eps=e), w4),
        "decode_gemv_w8_rows": (True, BF, 3072, lambda x, w, nw, e: ops.decode_gemv_w8_rows(x, *w, norm_w=nw, eps=e), w8),
        "decode_gemv_w4_rows": (True, BF, 3072, lambda x, w, nw, e: ops.decode_gemv_w4_rows(x, *w, norm_w=nw, eps=e), w4),
    }


def _decode_kernel(name, dt, K):
    """the kernel a decode projection launches (vg_decode.hip / vg_decode_w4.hip / vg_decode_mfma.hip, restated): vg_decode_gemv takes
    decode_gemv_fast_kernel when the row is 384 or 256 x {1, 2, 4, 7, 8} 16-byte chunks and decode_gemv_kernel otherwise; the others have one kernel"""
    if name.startswith("decode_gemv bf16") or name.startswith("decode_gemv fp32"):
        nch = K // (8 if dt == BF else 4)
        return "decode_gemv_fast_kernel" if nch == 384 or (nch % 256 == 0 and nch // 256 in (1, 2, 4, 7, 8)) else "decode_gemv_kernel"
    return {"decode_gemv_p13": "decode_gemv_fast_kernel P13", "decode_gemv_w8": "decode_gemv_fast_kernel W8", "decode_gemv_w4": "decode_gemv_w4_kernel",
            "decode_gemv_rows": "decode_gemv_rows_kernel", "decode_gemm_rows": "decode_gemm_rows_kernel", "decode_gemm_w8_rows": "decode_gemm_rows_kernel W8",
            "decode_gemm_w4_rows": "decode_gemm_rows_kernel W4", "decode_gemv_w8_rows": "decode_gemv_w8_rows_kernel",
            "decode_gemv_w4_rows": "decode_gemv_w4_rows_kernel"}[name.split()[0]]


PROJ = ["decode_gemv bf16 K=64", "decode_gemv bf16", "decode_gemv fp32", "decode_gemv_p13", "decode_gemv_w8", "decode_gemv_w4", "decode_gemv_rows K=2048", "decode_gemv_rows",
        "decode_gemm_rows", "decode_gemm_w8_rows", "decode_gemm_w4_rows", "decode_gemv_w8_rows", "decode_gemv_w4_rows"]


@pytest.mark.parametrize("name", PROJ)
def test_decode_projection_prologue(cuda, name):
    """the RMSNorm prologue of a decode projection: with W[n, pi(n)] = 1 the contraction is exact and the output is the prologue's normalised value
    (bf16: rounded to bf16 before the product, as vg_decode.hip's dec_pack does — the value of the stand-alone bf16 RMSNorm).  The smallest row
    length the *_supported() queries accept (3072; the 13-bit rows: 4096; the plain GEMV also at K = 64); the B-row forms at B = 1 and B = 16.
    Staging: thread t of 256 owns the 16-byte chunks t + 256 i of the row."""
    from videoglamm_amd import ops
    rowsv, dt, K, call, build = _projections()[name]
    assert ops.decode_gemv_w8_rows_supported(3072) and ops.decode_gemv_w4_rows_supported(3072) and ops.decode_gemm_rows_supported(256, 3072)
    assert ops.decode_gemm_w8_rows_supported(256, 3072) and ops.decode_gemm_w4_rows_supported(256, 3072) and ops.decode_gemv_p13_supported(4096)
    nv = 8 if dt == BF else 4
    N = min(K, 256)
    pi = _pi(K, 256, nv, N)
    w = tuple(t.to(cuda) for t in build(N, K, pi))
    nw = R.norm_weights(K)[0]
    if name == "decode_gemv_p13":
        p13 = ops.decode_pack13(w[0], raw_cap=False)
        call = lambda x, w_, nw_, e: ops.decode_gemv(x, w_[0], norm_w=nw_, eps=e, p13=p13)                  # noqa: E731
    for B in ((1, 16) if rowsv else (1,)):
        cases, gots = [], []
        for x, probes in R.build_norm_rounds(B, K, dt, True, 256, nv, seed=4 + B):
            got = call(x.to(cuda), w, nw.to(cuda), RMS_EPS)
            assert got.shape == (B, N)
            full = R.norm_case(f"{name} B={B}", x, nw, None, RMS_EPS, True, dt, route=_decode_kernel(name, dt, K), probes=probes)
            pick = lambda t: t[:, pi]                                                                       # noqa: E731
            cases.append(R.Case(full.name, [pick(r) for r in full.refs], [pick(u) for u in full.units], dt, cpu32=pick(full.cpu32),
                                counted=pick(full.counted) if full.counted is not None else None, route=full.route))
            gots.append(got.cpu().reshape(-1))
        R.check(R.cat_cases(cases[0].name, cases), torch.cat(gots))


def test_decode_qkv_rope_prologue(cuda):
    """vg_decode_qkv_rope at position 0 with cos = 1, sin = 0 (the rotation is the identity: x1 * 1 + (-x2) * 0) under a one-hot W: q and the
    appended K and V rows are the bf16 RMSNorm of x at the picked columns"""
    from videoglamm_amd import _lib, ops
    H, Hkv, D, K = E.QKV[0]
    assert _lib.load().vg_decode_qkv_rope_supported(H, Hkv, D, K, 1)
    N = (H + 2 * Hkv) * D
    pi = torch.cat([_pi(K, 256, 8, K), _pi(K, 256, 8, N - K)])
    w = _onehot(N, K, pi).to(cuda)
    nw = R.norm_weights(K)[0]
    cs = torch.cat([torch.ones(D // 2), torch.zeros(D // 2)]).to(cuda)
    cases, gots = [], []
    for x, probes in R.build_norm_rounds(1, K, BF, True, 256, 8, seed=11):
        kc = torch.full((4, Hkv, D), E.SENTINEL, dtype=BF, device=cuda)
        vc = torch.full((4, Hkv, D), E.SENTINEL, dtype=BF, device=cuda)
        q = ops.decode_qkv_rope(x.to(cuda), w, nw.to(cuda), RMS_EPS, kc, vc, cs, torch.zeros(1, dtype=torch.int32, device=cuda), H, Hkv, D)
        assert bool((kc[1:] == E.SENTINEL).all()) and bool((vc[1:] == E.SENTINEL).all())
        full = R.norm_case("decode_qkv_rope pos 0", x, nw, None, RMS_EPS, True, BF, route="decode_gemv_fast_kernel RoPE", probes=probes)
        pick = lambda t: t[:, pi]                                                                           # noqa: E731
        cases.append(R.Case(full.name, [pick(r) for r in full.refs], [pick(u) for u in full.units], BF, cpu32=pick(full.cpu32), counted=pick(full.counted),
                            route=full.route))
        gots.append(torch.cat([q.reshape(-1), kc[0].reshape(-1), vc[0].reshape(-1)]).cpu())
    R.check(R.cat_cases(cases[0].name, cases), torch.cat(gots))


@pytest.mark.parametrize("K", [64, 256])
def test_linear_rows_ln_prologue(cuda, K):
    """vg_gemm_rows' LayerNorm prologue (force_fused) at M = 64 + 3 under a one-hot W: the bf16 LayerNorm itself"""
    from videoglamm_amd import ops
    M, N = 64 + 3, 64
    pi = _pi(K, 64, 8, N)
    w = _onehot(N, K, pi).to(cuda)
    lw, lb = R.norm_weights(K)
    x, probes = R.build_norm_rounds(M, K, BF, False, 64, 8, seed=6)[0]
    got = ops.linear_rows(x.to(cuda), w, ln=(lw.to(cuda), lb.to(cuda), LN_EPS), force_fused=True)
    full = R.norm_case(f"linear_rows ln K={K}", x, lw, lb, LN_EPS, False, BF, route="gemm_rows64_kernel", probes=probes)
    case = R.Case(full.name, [full.refs[0][:, pi]], [full.units[0][:, pi]], BF, cpu32=full.cpu32[:, pi], counted=full.counted[:, pi], route=full.route)
    R.check(case, got.cpu())


@pytest.mark.parametrize("K", [144, 288])
def test_linear_ln_prologue(cuda, K):
    """vg_gemm_ln (the row-register route: 65536 + 41 rows, N = 144) under a one-hot W; the CPU compares the first 128 and the last 389 rows"""
    from videoglamm_amd import _lib, ops
    M, N = 65536 + 41, 144
    assert _lib.load().vg_gemm_route(M, N, K, ops.BF16, 0, 0) == 7
    pi = _pi(K, 8, 8, N)
    w = _onehot(N, K, pi).to(cuda)
    lw, lb = R.norm_weights(K)
    x, probes = R.build_norm_rounds(M, K, BF, False, 8, 8, seed=7)[0]
    got = ops.linear_ln(x.to(cuda), (lw.to(cuda), lb.to(cuda), LN_EPS), w)
    idx = _checked_rows(M)
    sub = {int((idx == r).nonzero()[0]): k for r, k in probes.items()}
    full = R.norm_case(f"linear_ln K={K}", x[idx], lw, lb, LN_EPS, False, BF, route="gemm_rr_kernel LN", probes=sub)
    case = R.Case(full.name, [full.refs[0][:, pi]], [full.units[0][:, pi]], BF, cpu32=full.cpu32[:, pi], counted=full.counted[:, pi], route=full.route)
    R.check(case, got.cpu()[idx])


def test_linear_ln_window_prologue(cuda):
    """the window form at test_gemm_ln_window's smallest shape: the LayerNorm of every token, window-partitioned (ws = 8 divides the grid: no padding)"""
    import _cpu_ops as ref
    from videoglamm_amd import ops
    B, H, W, ws, K, N = 2, 256, 256, 8, 144, 432
    pi = torch.cat([_pi(K, 8, 8, K), _pi(K, 8, 8, K), _pi(K, 8, 8, K)])
    w = _onehot(N, K, pi).to(cuda)
    lw, lb = R.norm_weights(K)
    x, probes = R.build_norm_rounds(B * H * W, K, BF, False, 8, 8, seed=8)[0]
    got = ops.linear_ln(x.view(B, H, W, K).to(cuda), (lw.to(cuda), lb.to(cuda), LN_EPS), w, window=(B, H, W, ws))
    rowid = ref.window_partition(torch.arange(B * H * W, dtype=torch.float32).view(B, H, W, 1), ws).reshape(-1).long()      # window order -> token
    keep = _checked_rows(B * H * W)                                          # window-order rows compared
    tok = rowid[keep]
    sub = {i: probes[int(t)] for i, t in enumerate(tok.tolist()) if int(t) in probes}
    full = R.norm_case("linear_ln window", x[tok], lw, lb, LN_EPS, False, BF, route="gemm_rr_kernel LN window", probes=sub)
    case = R.Case(full.name, [full.refs[0][:, pi]], [full.units[0][:, pi]], BF, cpu32=full.cpu32[:, pi], counted=full.counted[:, pi], route=full.route)
    R.check(case, got.reshape(-1, N).cpu()[keep])


def test_mlp_rows_prologue(cuda):
    """vg_mlp_rows (force) at C = 144, M = 100: (a) identity-block w1, zero bias, w2 = 0: the output is the residual x bit for bit; (b) test_mlp_rows'
    one-hot w2 (four hidden copies x 0.25: exact): y = x + bf16(gelu(bf16(LayerNorm(x)))), both intermediate roundings as the kernel documents them,
    checked at the model's bound (R.mlp_onehot_case)."""
    from videoglamm_amd import ops
    C, M = 144, 100
    H = 4 * C
    lw, lb = R.norm_weights(C)
    lw, lb = 1.0 + 0.1 * lw, 0.1 * lb
    x, probes = R.build_norm_rounds(M, C, BF, False, 8, 8, seed=9)[0]
    d = lambda t: t.to(cuda)          # noqa: E731
    eye1 = torch.zeros(H, C, dtype=BF)
    eye1[torch.arange(H), torch.arange(H) % C] = 1.0
    eye2 = torch.zeros(C, H, dtype=BF)
    eye2[torch.arange(H) % C, torch.arange(H)] = 0.25
    zb1, zb2 = torch.zeros(H), torch.zeros(C)
    lnd = (d(lw), d(lb), LN_EPS)
    y0 = ops.mlp_rows(d(x), lnd, d(eye1), d(zb1), d(torch.zeros(C, H, dtype=BF)), d(zb2), force=True)
    assert torch.equal(y0.cpu(), x), "w2 = 0: the residual alone"
    y = ops.mlp_rows(d(x), lnd, d(eye1), d(zb1), d(eye2), d(zb2), force=True)
    case = R.mlp_onehot_case("mlp_rows one-hot", x, lw, lb, LN_EPS, probes, route="mlp_rows_kernel")
    R.check(case, y.cpu())


# ------------------------------------------------------------------ C. activations
ACTS = (R.ACT_GELU, R.ACT_QUICK_GELU, R.ACT_RELU, R.ACT_SILU, R.ACT_SIGMOID)
_ACT = {1: "gelu", 2: "quick_gelu", 3: "relu", 4: "silu", 5: "sigmoid"}


def _check_act(name, x, act, got, route, counted=None):
    assert bool(torch.isfinite(got.float()).all()), f"{name}: a non-finite output (inf * 0 ?)"
    if act == R.ACT_RELU:
        print(f"ACC {name:58s} route {route:22s} torch.equal")
        assert torch.equal(got.cpu(), x.float().clamp_min(0.0).to(got.dtype)), name
        return
    case = R.act_case(name, x, act, got.dtype, route=route)
    if counted is not None:
        case.counted = counted if case.counted is None else (case.counted & counted)
    R.check(case, got.cpu())


@pytest.mark.parametrize("dt,odt", [(BF, BF), (F32, F32), (BF, F32), (F32, BF)], ids=["bf16", "fp32", "bf16-fp32", "fp32-bf16"])
def test_activation(cuda, dt, odt):
    from videoglamm_amd import ops
    x = R.act_grid(dt)
    for act in ACTS:
        _check_act(f"activation {_ACT[act]} {_NAME[dt]}->{_NAME[odt]}", x, act, ops.activation(x.to(cuda), act, out_dtype=odt), "act_kernel")


def _gu(dt):
    """gate | up rows: the gate walks the activation grid, up is random; a multiple of 8 columns"""
    g = R.act_grid(dt)
    Fh = 136
    M = g.numel() // Fh
    gate = g[:M * Fh].float().reshape(M, Fh)
    up = torch.randn(M, Fh, generator=torch.Generator().manual_seed(12)) * 2.0
    spec = torch.tensor([0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0])
    gate[0, :8] = spec
    return torch.cat([gate, up], dim=1).to(dt)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_swiglu(cuda, dt):
    from videoglamm_amd import ops
    gu = _gu(dt)
    got = ops.swiglu(gu.to(cuda))
    assert bool(torch.isfinite(got.float()).all())
    R.check(R.swiglu_case(f"swiglu {_NAME[dt]}", gu, route="swiglu_kernel"), got.cpu())


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_axpby(cuda, dt):
    """vector path (bf16, n and the period multiples of 8; b bf16 and fp32), scalar path (odd sizes, fp32, no b), broadcast b"""
    from videoglamm_amd import ops
    g = torch.Generator().manual_seed(13)
    a = (torch.randn(6, 50, 32, generator=g) * 3.0).to(dt)
    cases = [("vec b same dtype", a, (torch.randn(50, 32, generator=g)).to(dt), 1.0, 0.1), ("vec b fp32 row", a, torch.randn(32, generator=g), 2.0, 1.0),
             ("scalar odd", (torch.randn(7, 5, 3, generator=g)).to(dt), torch.randn(5, 3, generator=g).to(dt), 0.5, -1.5),
             ("scalar no b", a, None, 0.75, 3.0), ("add", a, a, 1.0, 1.0)]
    for name, aa, bb, al, be in cases:
        got = ops.axpby(aa.to(cuda), _d(bb, cuda), al, be)
        vec = dt == BF and bb is not None and aa.numel() % 8 == 0 and bb.numel() % 8 == 0
        R.check(R.axpby_case(f"axpby {name} {_NAME[dt]}", aa, bb, al, be, dt, route="axpby_vec_kernel" if vec else "axpby_kernel"), got.cpu())
    if dt == BF:
        got = ops.axpby(a.to(cuda), None, 1.0, 0.0, out_dtype=F32)
        assert torch.equal(got.cpu(), a.float())


@pytest.mark.parametrize("odt", [BF, F32], ids=["bf16", "fp32"])
def test_mask_for_mem(cuda, odt):
    import _cpu_ops as ref
    from videoglamm_amd import ops
    x = torch.cat([R.act_grid(F32), torch.randn(3 * 40 * 40, generator=torch.Generator().manual_seed(14)) * 4.0])
    x = x[torch.isfinite(x) & (x.abs() < 1e30)]
    got = ops.mask_for_mem(x.to(cuda), 1, 20.0, -10.0, odt)
    print(f"ACC mask_for_mem binarize {_NAME[odt]:40s} route mask_for_mem_kernel    torch.equal")
    assert torch.equal(got.cpu(), ref.mask_for_mem(x, 1, 20.0, -10.0, odt))
    got = ops.mask_for_mem(x.to(cuda), 0, 20.0, -10.0, odt)
    R.check(R.mask_sigmoid_case(f"mask_for_mem sigmoid {_NAME[odt]}", x, 20.0, -10.0, odt, route="mask_for_mem_kernel"), got.cpu())


def test_cast(cuda):
    """both directions, torch.equal: ties to even, the overflow to inf past the largest bf16, subnormals, signed zeros"""
    from videoglamm_amd import ops
    g = torch.Generator().manual_seed(15)
    bits = torch.randint(0, 2 ** 31 - 1, (1 << 16,), generator=g, dtype=torch.int64).to(torch.int32)
    x = torch.cat([bits.view(F32), -bits.view(F32), R.act_grid(F32),
                   torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.4e38, -3.4e38, 2.0 ** -133, 2.0 ** -134, 2.0 ** -140, 0.0, -0.0])])
    x = x[~torch.isnan(x)]
    print("ACC cast fp32 -> bf16 -> fp32                                    route cast_kernel            torch.equal")
    y = ops.cast(x.to(cuda), BF)
    assert torch.equal(y.cpu(), x.to(BF))
    assert torch.equal(ops.cast(y, F32).cpu(), x.to(BF).float())


def _epilogue_inputs(M, N, K):
    """x [M, K] whose first min(N, K) columns walk the activation grid (every grid point once in the first copy, which the share check counts;
    the shape must hold the whole grid), the one-hot W [N, K] with pi(n) = n mod K, and the counted mask of the output"""
    g = R.act_grid(BF)
    c = min(N, K)
    assert M * c >= g.numel(), "the shape does not hold the activation grid"
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)).to(BF)
    x[:, :c] = g.repeat(-(-M * c // g.numel()))[: M * c].reshape(M, c)
    pi = torch.arange(N) % K
    counted = (torch.arange(M * c) < g.numel()).reshape(M, c)[:, pi % c] & (torch.arange(N) < c)[None, :]
    return x, _onehot(N, K, pi), pi, counted


def _epilogue_body(cuda, name, shapes, route_ok):
    """the five activation codes as GEMM epilogues through ops.linear with a one-hot weight and no bias (the contraction is exact)"""
    from videoglamm_amd import ops
    n = 0
    for (M, N, K) in shapes:
        assert route_ok(M, N, K), (name, M, N, K)
        x, w, pi, counted = _epilogue_inputs(M, N, K)
        for act in ACTS:
            got = ops.linear(x.to(cuda), w.to(cuda), None, act)
            _check_act(f"linear epilogue {_ACT[act]} {name} {M}x{N}x{K}", x[:, pi], act, got, f"vg_gemm {name}", counted)
            n += 1
    return n


def _glu_body(cuda, name, M, F_, K, route):
    """the glu = True epilogue against the SwiGLU model: W = gate rows | up rows, both one-hot; the gate columns of x walk the activation grid
    up to +-100 (silu(gate) * up stays finite), the up columns are random"""
    from videoglamm_amd import _lib, ops
    assert _lib.load().vg_gemm_route(M, F_, K, 1, 1, 0) == route, (name, M, F_, K)
    assert K >= 2 * F_
    g = R.act_grid(BF)
    g = g[g.float().abs() <= 100.0]
    assert M * F_ >= g.numel(), "the shape does not hold the activation grid"          # (the grid is ordered: a part of it is a narrow range)
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)) * 2.0).to(BF)
    x[:, :F_] = g.repeat(-(-M * F_ // g.numel()))[: M * F_].reshape(M, F_)
    pg, pu = torch.arange(F_), F_ + (torch.arange(F_) * 7 + 3) % F_
    w = torch.cat([_onehot(F_, K, pg), _onehot(F_, K, pu)])
    got = ops.linear(x.to(cuda), w.to(cuda), glu=True)
    assert bool(torch.isfinite(got.float()).all())
    R.check(R.swiglu_case(f"linear glu epilogue {name} {M}x{F_}x{K}", torch.cat([x[:, pg], x[:, pu]], dim=1), route=f"vg_gemm {name} glu"), got.cpu())


def _route_is(route):
    from videoglamm_amd import _lib
    return lambda M, N, K: _lib.load().vg_gemm_route(M, N, K, 1, 0, 0) == route


@pytest.mark.parametrize("name", ["skinny", "k64b", "small64", "s128", "glds"])
def test_linear_epilogues(cuda, name, monkeypatch):
    route, env, shapes = E.LINEAR_ROUTES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # (VG_GEMM_SPLITK is read by ops.linear at every call)
    pick = {"skinny": [(16, 512, 2048), (16, 512, 14336)], "k64b": [(129, 136, 144)], "small64": [(129, 200, 256)], "s128": [(300, 200, 520)],
            "glds": [(129, 130, 1544)]}[name]
    assert all(s in shapes for s in pick)
    _epilogue_body(cuda, name, pick, _route_is(route))
    if name == "skinny":
        _glu_body(cuda, name, 16, 512, 2048, 0)
    if name == "glds":
        _glu_body(cuda, name, 129, 72, 1544, 1)


def _child_body(cuda, name):
    """what a child process runs under the route knob of _exact.LINEAR_ROUTES[name] (the knobs are read once per process)"""
    route, _, shapes = E.LINEAR_ROUTES[name]
    n = _epilogue_body(cuda, name, shapes[1:2] if name == "p8n" else shapes[:1], _route_is(route))          # (p8n: 777 x 384 x 320)
    if name == "p8":
        _glu_body(cuda, name, 300, 128, 576, 3)
    return n


@pytest.mark.parametrize("name", ["p8", "p8n", "rr"])
def test_linear_epilogues_forced_routes(cuda, name):
    """the 256 x 256, 256 x 192 and row-register kernels' epilogues: the knobs of test_gemm_route_knobs / test_linear_forced_routes, a child process each"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, torch; sys.path[:0] = [%r, %r]\n"
            "import test_rowwise_accuracy_gpu as t\n"
            "from videoglamm_amd import _lib\n"
            "assert _lib.load().vg_init(0) > 0\n"
            "print('rowwise ok', t._child_body(torch.device('cuda:0'), %r))\n") % (os.path.dirname(here), here, name)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **E.LINEAR_ROUTES[name][1]), capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "rowwise ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ D. rotations
def _llm_tables(n, D):
    ang = torch.arange(n)[:, None].float() * (1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)))[None]
    return ang.cos(), ang.sin()


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_rope_half(cuda, dt):
    """pos0 > 0 on a strided head view [S, H of H + 2, D]: bf16 bit for bit (every product rounded), fp32 by the element check; the heads outside
    the view untouched"""
    from videoglamm_amd import ops
    S, H, D, pos0 = 37, 6, 64, 11
    cos, sin = _llm_tables(100, D)
    big = torch.randn(S, H + 2, D, generator=torch.Generator().manual_seed(16)).to(dt)
    g = big.to(cuda)
    ops.rope_half_(g[:, :H], cos.to(cuda), sin.to(cuda), pos0)
    got = g.cpu()
    assert torch.equal(got[:, H:], big[:, H:])
    if dt == BF:
        print("ACC rope_half bf16                                               route rope_half_kernel       torch.equal")
        assert torch.equal(got[:, :H], R.rope_half_bf16(big[:, :H], cos, sin, pos0))
    else:
        R.check(R.rope_half_case("rope_half fp32", big[:, :H], cos, sin, pos0), got[:, :H])


@pytest.mark.parametrize("dt,C,route", [(BF, 64, "rope_axial_vec_kernel"), (BF, 36, "rope_axial_kernel"), (F32, 32, "rope_axial_kernel")], ids=["bf16-vec", "bf16-scalar", "fp32"])
def test_rope_axial(cuda, dt, C, route):
    """scalar and vector routes (vg_rope_axial: bf16 with C % 8 == 0 takes the vector kernel); n_rope = 2 n_grid so that tok % n_grid matters; the
    tokens past n_rope untouched bit for bit"""
    from videoglamm_amd import ops
    B, n_grid, extra = 2, 64, 8
    n_rope, N = 2 * n_grid, 2 * n_grid + extra
    assert (dt == BF and C % 8 == 0) == (route == "rope_axial_vec_kernel")
    g = torch.Generator().manual_seed(17)
    ang = torch.randn(n_grid, C // 2, generator=g) * 2.0
    cos, sin = ang.cos(), ang.sin()
    x = torch.randn(B, N, C, generator=g).to(dt)
    got = ops.rope_axial_(x.clone().to(cuda), cos.to(cuda), sin.to(cuda), n_rope, n_grid).cpu()
    assert torch.equal(got[:, n_rope:], x[:, n_rope:])
    R.check(R.rope_axial_case(f"rope_axial {_NAME[dt]} C={C}", x, cos, sin, n_rope, n_grid, route=route), got[:, :n_rope])


def test_rope_axial_heads(cuda):
    """q | k of a fused q|k|v row (two heads, row stride 3 C): each head against float64, equal to the per-head contiguous calls (kept from
    test_rope_axial_heads), v and the tokens past n_rope untouched"""
    from videoglamm_amd import ops
    B, N, C, n_grid, n_rope = 2, 70, 64, 32, 64
    g = torch.Generator().manual_seed(18)
    ang = torch.randn(n_grid, C // 2, generator=g) * 2.0
    cos, sin = ang.cos(), ang.sin()
    qkv = torch.randn(B, N, 3 * C, generator=g).to(BF)
    z = ops.rope_axial_heads_(qkv.clone().to(cuda), 2, cos.to(cuda), sin.to(cuda), n_rope, n_grid).cpu()
    assert torch.equal(z[..., 2 * C:], qkv[..., 2 * C:]) and torch.equal(z[:, n_rope:], qkv[:, n_rope:])
    for h in range(2):
        part = qkv[..., h * C:(h + 1) * C].contiguous()
        R.check(R.rope_axial_case(f"rope_axial_heads head {h}", part, cos, sin, n_rope, n_grid, route="rope_axial_vec_kernel"), z[:, :n_rope, h * C:(h + 1) * C])
        assert torch.equal(z[..., h * C:(h + 1) * C], ops.rope_axial_(part.to(cuda), cos.to(cuda), sin.to(cuda), n_rope, n_grid).cpu())


@pytest.mark.parametrize("dt,S,D,route", [(BF, 5, 64, "vec"), (BF, 1, 64, "scalar"), (BF, 5, 24, "scalar"), (F32, 5, 64, "scalar")],
                         ids=["bf16-vec", "bf16-one-row", "bf16-D24", "fp32"])
@pytest.mark.parametrize("use_dev", [False, True], ids=["pos0", "pos_dev"])
def test_rope_kv_append(cuda, dt, S, D, route, use_dev):
    """scalar and vec kernels (vg_rope_kv_append: bf16, D % 16 == 0, S > 1 take the vec kernel), position as an argument and from device memory: the
    rotation bit for bit in bf16 (element check in fp32), the appended cache rows equal, every other cache row untouched (sentinel), v copied"""
    from videoglamm_amd import ops
    H, Hkv, pos, max_len = 4, 2, 3, 16
    assert (dt == BF and D % 16 == 0 and S > 1) == (route == "vec")
    cos, sin = _llm_tables(max_len, D)
    qkv = torch.randn(S, (H + 2 * Hkv) * D, generator=torch.Generator().manual_seed(19)).to(dt)
    kc = torch.full((max_len, Hkv, D), E.SENTINEL, dtype=dt, device=cuda)
    vc = torch.full((max_len, Hkv, D), E.SENTINEL, dtype=dt, device=cuda)
    g = qkv.clone().to(cuda)
    pd = torch.tensor([pos], dtype=torch.int32, device=cuda) if use_dev else None
    ops.rope_kv_append_(g, kc, vc, cos.to(cuda), sin.to(cuda), H, Hkv, D, pos0=0 if use_dev else pos, pos_dev=pd)
    got, kc, vc = g.cpu(), kc.cpu(), vc.cpu()
    q0, k0 = qkv[:, : H * D].reshape(S, H, D), qkv[:, H * D:(H + Hkv) * D].reshape(S, Hkv, D)
    v0 = qkv[:, (H + Hkv) * D:].reshape(S, Hkv, D)
    assert torch.equal(got[:, H * D:], qkv[:, H * D:]), "the k | v columns of qkv are read only"
    assert torch.equal(vc[pos:pos + S], v0)
    for c in (kc, vc):
        assert bool((c[:pos] == E.SENTINEL).all()) and bool((c[pos + S:] == E.SENTINEL).all()), "a cache row outside [pos, pos + S) was written"
    gq, gk = got[:, : H * D].reshape(S, H, D), kc[pos:pos + S]
    if dt == BF:
        print(f"ACC rope_kv_append bf16 S={S} D={D} {'pos_dev' if use_dev else 'pos0':30s} route {route:22s} torch.equal")
        assert torch.equal(gq, R.rope_half_bf16(q0, cos, sin, pos)) and torch.equal(gk, R.rope_half_bf16(k0, cos, sin, pos))
    else:
        R.check(R.rope_half_case("rope_kv_append fp32 q", q0, cos, sin, pos), gq)
        R.check(R.rope_half_case("rope_kv_append fp32 k", k0, cos, sin, pos), gk)
