"""Exact-integer tests of every contraction kernel that has an exact form (-m gpu).  Operands are small integers (tests/_exact.py), so every fp32
partial sum is exact in any order: each result must equal the float64 reference BIT FOR BIT (bf16: its one round-to-nearest-even rounding).  Every
comparison in this file is torch.equal; there is no tolerance.  A lost, doubled or mis-paired product, a K tail dropped in the ragged rows only, a
block with its neighbour's scale all change the result by at least one unit.  Operand gaps (lda / ldw > K, guard rows) hold +-2^20, output buffers a
sentinel around the [M, N] view: reads past K and writes past M / N show as well.  A failure message says where to read (_exact.explain).

Covered — pytest cases per entry point (139 in all; a case loops over its shapes and variants), bf16 + fp32 where the kernel has both:
  ops.linear / vg_gemm ........ 26 cases: skinny (route 0) 14 = 7 M x 2 dtypes, 8 (N, K) each; k64b / s128 / glds (2 / 4 / 1) 6 = 3 x 2 dtypes on
                                12 / 2 / 2 shapes; small64 (5) 1 on 3 shapes; the forced 256x256 (3), 256x192 (6) and row-register (7) kernels 3, one
                                child process per knob, 3 / 3 / 2 shapes (the 256x256 ones batched x 3 as well); GLU 2.  Every shape: plain, bias + ReLU,
                                gamma + residual, fp32 output, strided + poisoned operands into a sentinel buffer (row-register: what that kernel takes).
                                VG_GEMM_SPLITK=0 wherever a tile kernel is meant (ops.linear's split-K rule would take the few-tile long-K shapes);
                                fp32 inputs take the 128x128 tile kernel their K selects (_exact.fp32_tile_route, asserted per shape)
  ops._linear_splitk .......... 6: 2 shapes x 3 dtype pairs, each ksplit 2, 3, 4, 8, contiguous and poisoned, the whole epilogue in the reducing pass,
                                also into a destination with sentinel rows before and after it
  ops.linear_window ........... 4: modes 1 and 2 on 2 geometries x 2 dtypes (padding rows: exactly the bias / never reach the image)
  ops.bmm_nt .................. 2: shared_a (a K-padded, poisoned A), batch > 1 on K = 32 / 64 / 72, the lane-per-column short-K kernel
  ops.linear_f8 ............... 6: 3 shapes x {bf16, fp32 out}, with and without residual, host-built e4m3 codes and power-of-two row scales, strided W
  ops.decode_gemv ............. 15 + 1: 8 K x 2 dtypes, N = 33, 257, 1001 (fp32 at K = 32768 does not fit the kernel's LDS staging: the launcher must
                                refuse it, test_decode_gemv_fp32_row_limit)
  ops.decode_gemv_w8 / _w4 .... 4 / 8: 4 K (w4: x 2 layouts), N = 33, 1001; scales that differ row to row / block to block
  ops.decode_gemv_rows / w8_rows  9 / 12: 3 B x 3 (4) K, N = 33, 1001 (where B x K exceeds the norm's LDS staging the launcher must refuse the fused norm)
                                every GEMV: plain, residual, RMSNorm-fused (bf16 input), GLU, poisoned x / W into a sentinel-guarded output; with fp32
                                output as well (plain, residual, sentinel) wherever the entry point has an out_dtype — all but decode_gemv_rows
  ops.decode_qkv_rope ......... 2: K = 2048, 4096 at H, Hkv = 16, 2: q (sentinel-guarded), the appended K / V row, the rest of the caches untouched
  ops.mlp3_grouped ............ 36: 18 (G, R, widths) x 2 output dtypes, bf16 rounding between the layers
  ops.linear_rows ............. 8 (K, N) without LayerNorm / RoPE: plain, ReLU, residual, A + A2, block-strided A
GLU forms: SiLU has no exact form, so they are compared bit for bit with ops.swiglu of the SAME kernel's non-GLU output over the 2N rows, which the
exact test has just pinned (one vg_silu definition serves every site).
Left out, because their arithmetic has no exact form: vg_gemm_ln, vg_mlp_rows, the LayerNorm / RoPE forms of vg_gemm_rows, the quantisers, and GELU /
SiLU / sigmoid epilogues (they stay with the tolerance tests of test_kernels_gpu.py and the rounding-level tests of test_rowwise_accuracy_gpu.py).
vg_twoway_image_update and vg_mask_upscale are in tests/test_decoder_fused_gpu.py: a selector design under which the two-way update's contractions
ARE exact, and float64 chains that round where the kernels round.

Wall time on one MI355X: 22 s for the 139 cases (the three child processes 2.3 - 2.7 s each, every other case under 1 s)."""
import os
import subprocess
import sys

import pytest
import torch

import _cpu_ops as ref
import _exact as E

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BF, F32 = torch.bfloat16, torch.float32
DT = [BF, F32]

VARIANTS = {          # bias, relu, gamma, res, f32 (output of a bf16 GEMM), strided (poisoned operands + sentinel output)
    "plain": {},
    "bias+relu": dict(bias=1, relu=1),
    "gamma+residual": dict(gamma=1, res=1),
    "fp32 out": dict(f32=1),
    "strided+poisoned": dict(bias=1, gamma=1, res=1, strided=1),
}
RR_VARIANTS = {       # what the row-register kernel takes: no LayerScale, no ReLU, bf16 out
    "plain": {},
    "bias": dict(bias=1),
    "bias+residual": dict(bias=1, res=1),
    "residual": dict(res=1),
    "strided+poisoned": dict(bias=1, res=1, strided=1),
}


def _lib():
    from videoglamm_amd import _lib as L
    return L.load()


def _check_linear(cuda, dtype, M, N, K, variants=VARIANTS):
    """ops.linear on one shape in every variant; returns the number of comparisons"""
    from videoglamm_amd import ops
    seed = 1000 * M + 10 * N + K
    x, w = E.ints((M, K), seed=seed), E.ints((N, K), seed=seed + 7)
    xd, wd = x.to(cuda, dtype), w.to(cuda, dtype)
    n = 0
    for name, v in variants.items():
        if v.get("f32") and dtype == F32:
            continue
        odt = F32 if v.get("f32") else dtype
        bias, gamma, res = E.epilogue_operands(M, N, seed, res_dtype=odt)
        bias, gamma, res = (bias if v.get("bias") else None), (gamma if v.get("gamma") else None), (res if v.get("res") else None)
        want = E.reference(x, w, bias, gamma, res, relu=bool(v.get("relu")), out_dtype=odt)
        d = lambda t: None if t is None else t.to(cuda)      # noqa: E731
        act = ops.ACT_RELU if v.get("relu") else ops.ACT_NONE
        what = f"linear {name} {str(dtype)[6:]} M={M} N={N} K={K}"
        if v.get("strided"):
            xb, wb = E.poisoned(x, dtype=dtype).to(cuda), E.poisoned(w, dtype=dtype).to(cuda)
            rb = None if res is None else E.poisoned(res.float(), pad=8, dtype=odt).to(cuda)
            big, view = E.sentinel_out(M, N, odt, cuda)
            got = ops.linear(xb[:M, :K], wb[:N, :K], d(bias), act, d(gamma), None if rb is None else rb[:M, :N], out_dtype=odt, out=view)
            assert got.data_ptr() == view.data_ptr()
            E.check(view, want, x, w, what)
            assert E.sentinel_intact(big, M, N), what + ": written outside [M, N]"
        else:
            E.check(ops.linear(xd, wd, d(bias), act, d(gamma), d(res), out_dtype=odt), want, x, w, what)
        n += 1
    return n


def _route_ok(M, N, K, dtype, route):
    got = _lib().vg_gemm_route(M, N, K, 1 if dtype == BF else 0, 0, 0)
    if dtype == BF or route == 0:
        return got == route
    return got == E.fp32_tile_route(K)          # fp32 has the 128x128 tile kernels only: which of them follows K x 4 bytes


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 8, 9, 16])
def test_linear_skinny(cuda, dtype, M):
    for (m, N, K) in E.LINEAR_ROUTES["skinny"][2]:
        if m == M:
            assert _route_ok(M, N, K, dtype, 0)
            _check_linear(cuda, dtype, M, N, K)


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", ["k64b", "s128", "glds"])
def test_linear_tile_routes(cuda, dtype, name, monkeypatch):
    route, env, shapes = E.LINEAR_ROUTES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # (VG_GEMM_SPLITK is read by ops.linear at every call)
    for (M, N, K) in shapes:
        assert _route_ok(M, N, K, dtype, route), (name, M, N, K)
        _check_linear(cuda, dtype, M, N, K)


def test_linear_small64(cuda):
    route, _, shapes = E.LINEAR_ROUTES["small64"]
    for (M, N, K) in shapes:
        assert _route_ok(M, N, K, BF, route)
        _check_linear(cuda, BF, M, N, K)


def _check_glu(cuda, dtype, M, F_, K):
    """linear(glu=True) == vg_swiglu of the same kernel family's [M, 2F] output, which is itself exact"""
    from videoglamm_amd import ops
    x, w = E.ints((M, K), seed=M + K), E.ints((2 * F_, K), seed=F_ + K)
    xd, wd = x.to(cuda, dtype), w.to(cuda, dtype)
    gu = ops.linear(xd, wd)
    E.check(gu, E.reference(x, w, out_dtype=dtype), x, w, f"linear (gate | up rows) M={M} F={F_} K={K}")
    y = ops.linear(xd, wd, glu=True)
    assert y.shape == (M, F_) and torch.equal(y, ops.swiglu(gu)), f"GLU epilogue M={M} F={F_} K={K}: " + E.explain(y, ops.swiglu(gu).cpu())


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_linear_glu(cuda, dtype, monkeypatch):
    monkeypatch.setenv("VG_GEMM_SPLITK", "0")
    for (M, F_, K) in ((1, 40, 72), (5, 96, 2048), (16, 33, 328), (129, 72, 1544), (40, 96, 328)):
        # <= 16 rows: the skinny kernel's GLU epilogue; above: the 128-byte-step tile kernel with gate | up halves (the short-K kernels have no GLU form)
        assert _lib().vg_gemm_route(M, F_, K, 1 if dtype == BF else 0, 1, 0) == (0 if M <= 16 else 1), (M, F_, K)
        _check_glu(cuda, dtype, M, F_, K)


def _child_body(cuda, name):
    """what a child process runs under the knob of LINEAR_ROUTES[name] (the knobs are read once per process)"""
    from videoglamm_amd import ops
    route, _, shapes = E.LINEAR_ROUTES[name]
    n = 0
    for (M, N, K) in shapes:
        assert _route_ok(M, N, K, BF, route), (name, M, N, K, _lib().vg_gemm_route(M, N, K, 1, 0, 0))
        n += _check_linear(cuda, BF, M, N, K, RR_VARIANTS if name == "rr" else VARIANTS)
        if name == "p8":              # batched: a workgroup of the persistent kernel walks several tiles of several entries
            a, w = E.ints((3, M, K), seed=M), E.ints((3, N, K), seed=N)
            y = ops.bmm_nt(a.to(cuda, BF), w.to(cuda, BF))
            for b in range(3):
                E.check(y[b], E.reference(a[b], w[b], out_dtype=BF), a[b], w[b], f"bmm_nt (p8) entry {b} M={M} N={N} K={K}")
            n += 3
    if name == "p8":
        assert _lib().vg_gemm_route(300, 128, 576, 1, 1, 0) == 3
        _check_glu(cuda, BF, 300, 128, 576)
    return n


def _run_child(name):
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, torch; sys.path[:0] = [%r, %r]\n"
            "import test_contraction_exact_gpu as t\n"
            "from videoglamm_amd import _lib\n"
            "assert _lib.load().vg_init(0) > 0\n"
            "print('exact ok', t._child_body(torch.device('cuda:0'), %r))\n") % (os.path.dirname(here), here, name)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **E.LINEAR_ROUTES[name][1]), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "exact ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("name", ["p8", "p8n", "rr"])
def test_linear_forced_routes(cuda, name):
    """the 256x256, 256x192 and row-register kernels on shapes the rule never sends them: VG_GEMM_P8 = 2 / 3, VG_GEMM_RR = 2 in a child process each"""
    _run_child(name)


@pytest.mark.parametrize("in_dt,out_dt", [(BF, BF), (BF, F32), (F32, F32)], ids=["bf16", "bf16-fp32", "fp32"])
@pytest.mark.parametrize("M,N,K", [(40, 136, 4160), (213, 264, 14336)])
def test_linear_splitk(cuda, in_dt, out_dt, M, N, K):
    """vg_gemm_splitk directly: every ksplit, the whole epilogue in the reducing pass, contiguous and strided + poisoned operands"""
    from videoglamm_amd import ops
    x, w = E.ints((M, K), seed=K), E.ints((N, K), seed=K + 1)
    bias, gamma, res = E.epilogue_operands(M, N, K, res_dtype=out_dt)
    want = E.reference(x, w, bias, gamma, res, relu=True, out_dtype=out_dt)
    xb, wb = E.poisoned(x, dtype=in_dt).to(cuda), E.poisoned(w, dtype=in_dt).to(cuda)
    for xs, ws_ in ((x.to(cuda, in_dt), w.to(cuda, in_dt)), (xb[:M, :K], wb[:N, :K])):
        x2, m, lda = ops._rows2d(xs)
        for ks in (2, 3, 4, 8):
            got = ops._linear_splitk(_lib(), xs, x2, m, lda, ws_, bias.to(cuda), ops.ACT_RELU, gamma.to(cuda), res.to(cuda), out_dt, ks)
            E.check(got, want, x, w, f"splitk ks={ks} lda={lda} M={M} N={N} K={K}")
            big = torch.full((M + 4, N), E.SENTINEL, dtype=out_dt, device=cuda)          # the destination is contiguous rows: guard rows before and after it
            ops._linear_splitk(_lib(), xs, x2, m, lda, ws_, bias.to(cuda), ops.ACT_RELU, gamma.to(cuda), res.to(cuda), out_dt, ks, out=big[2:2 + M])
            E.check(big[2:2 + M], want, x, w, f"splitk into a guarded destination ks={ks} lda={lda} M={M} N={N} K={K}")
            assert bool((big[:2] == E.SENTINEL).all()) and bool((big[2 + M:] == E.SENTINEL).all()), f"splitk ks={ks}: written outside the M rows"


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,ws,K,N", E.WINDOWS)
def test_linear_window(cuda, dtype, B, H, W, ws, K, N):
    """mode 1 (gather): padding rows hold exactly the bias.  mode 2 (scatter + residual): the padding rows of the window-order input hold the
    poison and must not reach the image."""
    from videoglamm_amd import ops
    x, w = E.ints((B * H * W, K), seed=H), E.ints((N, K), seed=W)
    bias, gamma, _ = E.epilogue_operands(1, N, K)
    xw = ref.window_partition(x.view(B, H, W, K), ws)                 # zero rows where the grid is padded
    Mw = xw.shape[0] * ws * ws
    pad_rows = (xw.reshape(Mw, K).abs().sum(1) == 0)
    assert int(pad_rows.sum()) == Mw - B * H * W
    want = E.reference(xw.reshape(Mw, K), w, bias, relu=True, out_dtype=dtype)
    assert torch.equal(want[pad_rows].float(), bias.clamp_min(0)[None].expand(int(pad_rows.sum()), N).to(dtype).float())
    y = ops.linear_window(x.view(B, H, W, K).to(cuda, dtype), w.to(cuda, dtype), bias.to(cuda), B, H, W, ws, scatter=False, act=ops.ACT_RELU)
    E.check(y, want.view(-1, ws * ws, N), xw.reshape(Mw, K), w, f"window gather + ReLU {B, H, W, ws, K, N}")
    want0 = E.reference(xw.reshape(Mw, K), w, bias, out_dtype=dtype)                # no activation: the padding rows hold the bias itself, every column non-zero
    assert bool((bias != 0).all()) and torch.equal(want0[pad_rows].float(), bias[None].expand(int(pad_rows.sum()), N))
    y0 = ops.linear_window(x.view(B, H, W, K).to(cuda, dtype), w.to(cuda, dtype), bias.to(cuda), B, H, W, ws, scatter=False)
    E.check(y0, want0.view(-1, ws * ws, N), xw.reshape(Mw, K), w, f"window gather {B, H, W, ws, K, N}")
    assert torch.equal(y0.view(Mw, N).cpu()[pad_rows].float(), bias[None].expand(int(pad_rows.sum()), N)), "padding rows must hold exactly the bias"
    # mode 2: window-order rows [Mw, N2 = K] -> image order, + residual; N plays K here
    w2 = E.ints((K, N), seed=7)
    h = E.ints((Mw, N), seed=8)
    res = E.ints((B * H * W, K), (-8, -3, 1, 6), seed=9).to(dtype)
    full = E.reference(h, w2, None, E.pow2(K, seed=3), None, out_dtype=F32)
    img = ref.window_unpartition(full.view(-1, ws * ws, K), ws, B, H, W).reshape(B * H * W, K)
    want2 = (img.double() + res.double()).float().to(dtype)
    hp = h.clone()
    hp[pad_rows] = E.POISON
    z = ops.linear_window(hp.view(-1, ws * ws, N).to(cuda, dtype), w2.to(cuda, dtype), None, B, H, W, ws, scatter=True, gamma=E.pow2(K, seed=3).to(cuda),
                          residual=res.view(B, H, W, K).to(cuda))
    E.check(z, want2.view(B, H, W, K), None, None, f"window scatter {B, H, W, ws, K, N}")


@pytest.mark.parametrize("dtype", DT, ids=["bf16", "fp32"])
def test_bmm_nt(cuda, dtype):
    from videoglamm_amd import ops
    for (B, M, N, K) in E.BMM:
        odt = F32 if K == 32 else None
        a, w = E.ints((B, M, K), seed=M), E.ints((B, N, K), seed=N)
        y = ops.bmm_nt(a.to(cuda, dtype), w.to(cuda, dtype), out_dtype=odt)
        for b in range(B):
            E.check(y[b], E.reference(a[b], w[b], out_dtype=odt or dtype), a[b], w[b], f"bmm_nt entry {b} of {B, M, N, K}")
    M, N, K = E.BMM_SHARED                                            # shared_a: ONE K-padded A (its gap and guard rows poisoned) for every entry
    a, w = E.ints((M, K), seed=1), E.ints((3, N, K), seed=2)
    ab = E.poisoned(a, dtype=dtype, guard=0).to(cuda)
    y = ops.bmm_nt(ab, w.to(cuda, dtype), shared_a=True)
    for b in range(3):
        E.check(y[b], E.reference(a, w[b], out_dtype=dtype), a, w[b], f"bmm_nt shared_a entry {b}")


@pytest.mark.parametrize("out_dt", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K", E.F8)
def test_linear_f8(cuda, out_dt, M, N, K):
    """e4m3 codes of {-2, -1, 1, 2} and power-of-two row scales on both operands, built here (no quantiser); W strided with +-224 / 448 in its gap"""
    from videoglamm_amd import ops
    x, w = E.ints((M, K), seed=M), E.ints((N, K), seed=N)
    qs, ws_ = E.pow2(M, (-3, -1, 0, 2), seed=1), E.pow2(N, (-2, 0, 1, 3), seed=2)
    q = E.e4m3_codes(x).to(cuda)
    w8c = E.e4m3_codes(w).to(cuda)
    w8b = E.e4m3_codes(E.poisoned(w, poison=224.0)).to(cuda)
    res = E.ints((M, N), (-8, -3, 1, 6), seed=3).to(out_dt)
    xs, wsc = x * qs[:, None], w * ws_[:, None]
    for r in (None, res):
        want = E.reference(xs, wsc, residual=r, out_dtype=out_dt, unit=2.0 ** -5)
        for w8 in (w8c, w8b[:N, :K]):
            got = ops.linear_f8(q, qs.to(cuda), w8, ws_.to(cuda), residual=None if r is None else r.to(cuda), out_dtype=out_dt)
            E.check(got, want, xs, wsc, f"linear_f8 M={M} N={N} K={K} residual={r is not None} ldw={w8.stride(0)}")


# ---- decode GEMVs
def _row_buffers(cuda, x, N, odt, in_dt):
    """x [B, K] inside a poisoned buffer (row stride K + 16, 64 poisoned elements in front), and a sentinel-guarded [B, N] output"""
    B, K = x.shape
    flat = torch.full((64 + B * (K + 16) + 64,), E.POISON, dtype=F32)
    body = flat[64:64 + B * (K + 16)].view(B, K + 16)
    body[:, :K] = x
    flat = flat.to(cuda, in_dt)
    xv = flat[64:64 + B * (K + 16)].view(B, K + 16)[:, :K]
    n8 = (N + 7) // 8 * 8
    obig = torch.full((64 + B * (n8 + 8) + 64,), E.SENTINEL, dtype=odt, device=cuda)
    ov = obig[64:64 + B * (n8 + 8)].view(B, n8 + 8)[:, :N]
    return xv, obig, ov


def _out_intact(obig, ov):
    c = obig.clone()
    c[64:64 + ov.shape[0] * ov.stride(0)].view(ov.shape[0], ov.stride(0))[:, :ov.shape[1]] = E.SENTINEL
    return bool((c == E.SENTINEL).all())


def _gemv_variants(cuda, fn, in_dt, x, xn, nw, w_ref, wargs, wargs_strided, N, what, unit=1.0, f32_out=True, norm=True):
    """one GEMV entry point on one weight matrix.  fn(x, *wargs, **kw); x [B, K] integers, xn [B, K] in {-1, 1} with norm weights nw in {1, 2};
    w_ref [2N, K] the matrix the weights mean (rows N.. are the up rows of the GLU form).  f32_out: the entry point takes out_dtype (every one but
    decode_gemv_rows): fp32 output with and without residual, and into a sentinel-guarded fp32 destination."""
    from videoglamm_amd import ops
    B, K = x.shape
    eps = 1e-5
    # x * rsqrt(mean(x^2) + eps) = +-(1 - 5e-6) rounds to +-1 in bf16 for any 1-ulp rsqrt; times {1, 2}: exact
    xe = xn * nw[None, :]
    base = E.reference(torch.cat([x, xe]), w_ref, unit=unit)                        # [2B, 2N] exact fp32
    y_plain, y_norm = base[:B], base[B:]
    res = {dt: E.ints((B, N), (-8, -3, 1, 6), seed=N).to(dt) for dt in (BF, F32)}
    xd, xnd, nwd = x.to(cuda, in_dt), xn.to(cuda, in_dt), nw.to(cuda)
    half = lambda wa: tuple(a[:N] if (torch.is_tensor(a) and a.shape[0] == 2 * N) else a for a in wa)      # noqa: E731
    n = 0
    got = fn(xd, *half(wargs))
    E.check(got, y_plain[:, :N].to(in_dt), x, w_ref[:N], what + " plain")
    r = res[in_dt]
    got = fn(xd, *half(wargs), residual=r.to(cuda))
    E.check(got, (y_plain[:, :N].double() + r.double()).float().to(in_dt), x, w_ref[:N], what + " residual")
    n += 2
    if f32_out and in_dt == BF:
        E.check(fn(xd, *half(wargs), out_dtype=F32), y_plain[:, :N], x, w_ref[:N], what + " fp32 out")
        got = fn(xd, *half(wargs), residual=res[F32].to(cuda), out_dtype=F32)
        E.check(got, (y_plain[:, :N].double() + res[F32].double()).float(), x, w_ref[:N], what + " fp32 out + residual")
        n += 2
    if norm and in_dt == BF:
        got = fn(xnd, *half(wargs), norm_w=nwd, eps=eps)
        E.check(got, y_norm[:, :N].to(BF), xe, w_ref[:N], what + " norm")
        n += 1
    # poisoned x / W buffers, sentinel-guarded output, norm + residual where the form exists
    use_norm = norm and in_dt == BF
    xv, obig, ov = _row_buffers(cuda, xn if use_norm else x, N, in_dt, in_dt)
    kw = dict(norm_w=nwd, eps=eps) if use_norm else {}
    out = ov
    fn(xv, *half(wargs_strided), residual=r.to(cuda), out=out, **kw)
    want = ((y_norm if use_norm else y_plain)[:, :N].double() + r.double()).float().to(in_dt)
    E.check(out, want, xe if use_norm else x, w_ref[:N], what + " poisoned + sentinel")
    assert _out_intact(obig, ov), what + ": written outside the output"
    n += 1
    if f32_out and in_dt == BF:
        _, obig, ov = _row_buffers(cuda, x, N, F32, in_dt)
        fn(xv, *half(wargs_strided), residual=res[F32].to(cuda), out=ov, out_dtype=F32, **kw)
        want = ((y_norm if use_norm else y_plain)[:, :N].double() + res[F32].double()).float()
        E.check(ov, want, xe if use_norm else x, w_ref[:N], what + " poisoned + sentinel, fp32 out")
        assert _out_intact(obig, ov), what + ": written outside the fp32 output"
        n += 1
    # GLU: bitwise vg_swiglu of this kernel's own 2N-row output (just pinned above for the first N rows; here for all 2N)
    gu = fn(xd, *wargs)
    E.check(gu, y_plain.to(in_dt), x, w_ref, what + " gate | up rows")
    y = fn(xd, *wargs, glu=True)
    assert torch.equal(y, ops.swiglu(gu)), what + " GLU: " + E.explain(y, ops.swiglu(gu).cpu())
    n += 2
    return n


# (K = 32768 in bf16 only: vg_decode_gemv stages the row in 64 KB of LDS, an fp32 row of that length is not taken)
@pytest.mark.parametrize("dtype,K", [(dt, K) for K in E.GEMV_K for dt in DT if K * (2 if dt == BF else 4) <= 64 * 1024],
                         ids=lambda v: {BF: "bf16", F32: "fp32"}.get(v, str(v)))
def test_decode_gemv(cuda, dtype, K):
    from videoglamm_amd import ops
    x, xn, nw = E.ints((1, K), seed=K), E.ints((1, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in E.GEMV_N:
        w = E.ints((2 * N, K), seed=N + K)
        wd = w.to(cuda, dtype)
        wb = E.poisoned(w, dtype=dtype).to(cuda)[:2 * N, :K]
        _gemv_variants(cuda, ops.decode_gemv, dtype, x, xn, nw, w, (wd,), (wb,), N, f"decode_gemv {str(dtype)[6:]} N={N} K={K}")


def test_decode_gemv_fp32_row_limit(cuda):
    """K = 32768 in fp32 is the one (dtype, K) of the list vg_decode_gemv does not take (the row is staged in 64 KB of LDS): it must say so"""
    from videoglamm_amd import ops
    from videoglamm_amd._lib import VGKernelError
    K = 32768
    assert K in E.GEMV_K
    with pytest.raises(VGKernelError):
        ops.decode_gemv(torch.ones(1, K, device=cuda), torch.ones(33, K, device=cuda))
    E.check(ops.decode_gemv(torch.ones(1, K // 2, device=cuda), torch.ones(33, K // 2, device=cuda)), torch.full((1, 33), K / 2.0), None, None, "fp32 K = 16384")


def _w8(N, K, seed):
    w = E.ints((2 * N, K), seed=seed)
    sc = torch.ldexp(torch.ones(2 * N), ((torch.arange(2 * N) * 3) % 4 - 2).to(torch.int32))        # 2^-2 ... 2^1, different in neighbouring rows
    assert bool((sc[1:] != sc[:-1]).all())
    return w, sc


@pytest.mark.parametrize("K", E.GEMV_Q_K)
def test_decode_gemv_w8(cuda, K):
    from videoglamm_amd import ops
    x, xn, nw = E.ints((1, K), seed=K), E.ints((1, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in E.GEMV_Q_N:
        w, sc = _w8(N, K, N + K)
        codes, codes_b = E.e4m3_codes(w).to(cuda), E.e4m3_codes(E.poisoned(w, poison=224.0)).to(cuda)[:2 * N, :K]
        scd = sc.to(cuda)

        def fn(xx, w8, s, **kw):
            return ops.decode_gemv_w8(xx, w8, s[: w8.shape[0]].contiguous(), **kw)
        _gemv_variants(cuda, fn, BF, x, xn, nw, w * sc[:, None], (codes, scd), (codes_b, scd), N, f"decode_gemv_w8 N={N} K={K}", unit=0.25)


@pytest.mark.parametrize("layout", ["packed", "separate"])
@pytest.mark.parametrize("K", E.GEMV_Q_K)
def test_decode_gemv_w4(cuda, K, layout):
    """MXFP4 rows built here: block scales 2^0 .. 2^3 that differ between neighbouring blocks and between block 64 u + lane and 64 (u + 1) + lane
    (the packed head's walk), 2^0 blocks in every row, and one block per row with the scale byte 0 under non-zero codes: it contributes nothing"""
    from videoglamm_amd import ops
    x, xn, nw = E.ints((1, K), seed=K), E.ints((1, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in E.GEMV_Q_N:
        codes, scales, deq, _ = E.mxfp4_rows(2 * N, K, seed=N + K)
        live = (scales != 0).repeat_interleave(32, dim=1)
        assert torch.equal(ops.mxfp4_dequant(codes, scales)[live], deq[live])
        rows_ = ops.mxfp4_pack(codes, scales) if layout == "packed" else codes
        big = torch.full((2 * N + 2, rows_.shape[1] + 16), 0x77, dtype=torch.uint8)          # gap bytes and guard rows: two +6 codes each
        big[:2 * N, :rows_.shape[1]] = rows_
        strided = big.to(cuda)[:2 * N, :rows_.shape[1]]
        wargs = (rows_.to(cuda),) if layout == "packed" else (rows_.to(cuda), scales.to(cuda))
        wargs_b = (strided,) + wargs[1:]
        _gemv_variants(cuda, ops.decode_gemv_w4, BF, x, xn, nw, deq, wargs, wargs_b, N, f"decode_gemv_w4 {layout} N={N} K={K}")


def _rows_norm_fits(B, K):
    """the B-row kernels stage the whole rows of their bucket (1, 2, 4, 8, 16 rows) in LDS for the RMSNorm: 152 KB (the launchers' documented rule)"""
    br = next(b for b in (1, 2, 4, 8, 16) if B <= b)
    return br * K * 2 <= 160 * 1024 - 8 * 1024


def _rows_norm_refused(cuda, fn, B, K, *wargs):
    """where the norm-fused B-row form does not exist the launcher says so (no quiet fall-back): the other variants still run"""
    from videoglamm_amd._lib import VGKernelError
    with pytest.raises(VGKernelError):
        fn(torch.ones(B, K, dtype=BF, device=cuda), *wargs, norm_w=torch.ones(K, device=cuda), eps=1e-5)


@pytest.mark.parametrize("B", E.ROWS_B)
@pytest.mark.parametrize("K", E.ROWS_K)
def test_decode_gemv_rows(cuda, B, K):
    from videoglamm_amd import ops
    fits = _rows_norm_fits(B, K)
    x, xn, nw = E.ints((B, K), seed=K + B), E.ints((B, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in E.GEMV_Q_N:
        w = E.ints((2 * N, K), seed=N + K)
        wb = E.poisoned(w, dtype=BF).to(cuda)[:2 * N, :K]
        _gemv_variants(cuda, ops.decode_gemv_rows, BF, x, xn, nw, w, (w.to(cuda, BF),), (wb,), N, f"decode_gemv_rows B={B} N={N} K={K}", f32_out=False, norm=fits)
        if not fits:
            _rows_norm_refused(cuda, ops.decode_gemv_rows, B, K, wb[:N])


@pytest.mark.parametrize("B", E.W8_ROWS_B)
@pytest.mark.parametrize("K", E.GEMV_Q_K)
def test_decode_gemv_w8_rows(cuda, B, K):
    from videoglamm_amd import ops
    assert ops.decode_gemv_w8_rows_supported(K)
    fits = _rows_norm_fits(B, K)
    x, xn, nw = E.ints((B, K), seed=K + B), E.ints((B, K), (-1, 1), seed=K + 1), E.ints((K,), (1, 2), seed=K + 2)
    for N in E.GEMV_Q_N:
        w, sc = _w8(N, K, N + K)
        codes, codes_b = E.e4m3_codes(w).to(cuda), E.e4m3_codes(E.poisoned(w, poison=224.0)).to(cuda)[:2 * N, :K]
        scd = sc.to(cuda)

        def fn(xx, w8, s, **kw):
            return ops.decode_gemv_w8_rows(xx, w8, s[: w8.shape[0]].contiguous(), **kw)
        _gemv_variants(cuda, fn, BF, x, xn, nw, w * sc[:, None], (codes, scd), (codes_b, scd), N, f"decode_gemv_w8_rows B={B} N={N} K={K}", unit=0.25,
                       norm=fits)
        if not fits:
            _rows_norm_refused(cuda, fn, B, K, codes[:N], scd)


@pytest.mark.parametrize("H,Hkv,D,K", E.QKV)
def test_decode_qkv_rope(cuda, H, Hkv, D, K):
    """RMSNorm -> q|k|v -> RoPE -> append with (cos, sin) pairs from {(1, 0), (0, 1), (0, -1), (-1, 0)}: the rotation is a signed swap of the halves of a
    head, so q and the appended K row are the exact GEMV values moved and negated; V is the plain GEMV; every other cache row keeps its sentinel."""
    from videoglamm_amd import ops
    max_len, pos = 40, 17
    assert _lib().vg_decode_qkv_rope_supported(H, Hkv, D, K, 1)
    rows = (H + 2 * Hkv) * D
    xn, nw = E.ints((1, K), (-1, 1), seed=K), E.ints((K,), (1, 2), seed=K + 2)
    w = E.ints((rows, K), seed=K + 3)
    xe = xn * nw[None]
    acc = E.reference(xe, w)[0]                                                    # exact fp32 [rows]
    pair = torch.tensor([(1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-1.0, 0.0)])[torch.randint(4, (D // 2,), generator=torch.Generator().manual_seed(5))]
    c, s = pair[:, 0], pair[:, 1]

    def rot(v):                                                                     # rotate-half on [heads, D]
        a, b = v[:, : D // 2], v[:, D // 2:]
        return torch.cat([a * c - b * s, b * c + a * s], dim=1)
    q_want = rot(acc[: H * D].view(H, D)).to(BF).view(1, H * D)
    k_want = rot(acc[H * D:(H + Hkv) * D].view(Hkv, D)).to(BF)
    v_want = acc[(H + Hkv) * D:].view(Hkv, D).to(BF)
    kc = torch.full((max_len, Hkv, D), E.SENTINEL, dtype=BF, device=cuda)
    vc = torch.full((max_len, Hkv, D), -E.SENTINEL, dtype=BF, device=cuda)
    wb = E.poisoned(w, dtype=BF).to(cuda)[:rows, :K]
    for wd in (w.to(cuda, BF), wb):
        kc.fill_(E.SENTINEL), vc.fill_(-E.SENTINEL)
        qbig = torch.full((64 + H * D + 64,), E.SENTINEL, dtype=BF, device=cuda)           # q goes into a sentinel-guarded destination
        q = ops.decode_qkv_rope(xn.to(cuda, BF), wd, nw.to(cuda), 1e-5, kc, vc, torch.cat([c, s]).to(cuda), torch.tensor([pos], dtype=torch.int32, device=cuda),
                                H, Hkv, D, out=qbig[64:64 + H * D].view(1, H * D))
        what = f"decode_qkv_rope K={K} ldw={wd.stride(0)}"
        E.check(q, q_want, None, None, what + " q")
        assert bool((qbig[:64] == E.SENTINEL).all()) and bool((qbig[64 + H * D:] == E.SENTINEL).all()), what + ": written outside q"
        E.check(kc[pos], k_want, None, None, what + " appended K row")
        E.check(vc[pos], v_want, xe, w[(H + Hkv) * D:], what + " appended V row")
        keep = torch.ones(max_len, dtype=torch.bool)
        keep[pos] = False
        assert bool((kc.cpu()[keep] == E.SENTINEL).all()) and bool((vc.cpu()[keep] == -E.SENTINEL).all()), what + ": another cache row was written"


@pytest.mark.parametrize("out_dt", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("G,R,K,Hd,No", E.MLP3)
def test_mlp3_grouped(cuda, out_dt, G, R, K, Hd, No):
    """+-1 weights, integer biases, no sigmoid: three exact layers with ReLU and one bf16 rounding between them (partial sums are integers far below 2^24,
    proved per layer by the guard); token rows 1 .. G of a wider tensor, a wider sentinel-filled destination"""
    from videoglamm_amd import ops
    x = E.ints((R, G + 2, K), seed=R + K)
    x[:, 0] = E.POISON                                      # the token rows beside the heads' rows 1 .. G: never read
    x[:, G + 1] = -E.POISON
    w0, w1, w2 = E.ints((G, Hd, K), (-1, 1), seed=1), E.ints((G, Hd, Hd), (-1, 1), seed=2), E.ints((G, No, Hd), (-1, 1), seed=3)
    b0, b1, b2 = E.ints((G, Hd), (-3, -1, 2, 5), seed=4), E.ints((G, Hd), (-3, -1, 2, 5), seed=5), E.ints((G, No), (-3, -1, 2, 5), seed=6)
    out = torch.full((R, G, No + 3), E.SENTINEL, dtype=out_dt, device=cuda)
    c = lambda t: t.to(cuda)      # noqa: E731
    b = lambda t: t.to(cuda, BF)      # noqa: E731
    ops.mlp3_grouped(b(x)[:, 1:], G, ops.mlp3_pack(b(w0)), c(b0), ops.mlp3_pack(b(w1)), c(b1), ops.mlp3_pack(b(w2)), c(b2), out, 0)
    got = out.cpu()
    assert bool((got[:, :, No:] == E.SENTINEL).all())
    for g in range(G):
        h1 = E.reference(x[:, 1 + g], w0[g], b0[g], relu=True, out_dtype=BF).float()
        h2 = E.reference(h1, w1[g], b1[g], relu=True, out_dtype=BF).float()
        want = E.reference(h2, w2[g], b2[g], out_dtype=out_dt)
        E.check(got[:, g, :No], want, h2, w2[g], f"mlp3_grouped head {g} of {G, R, K, Hd, No}")


@pytest.mark.parametrize("M,N,K", E.LINEAR_ROWS)
def test_linear_rows(cuda, M, N, K):
    """vg_gemm_rows without LayerNorm / RoPE (bf16): plain, ReLU, residual, the A + A2 prologue (a2 repeated over blocks of M / 3 rows), the
    block-strided [B, rows, K] view of a poisoned buffer; every form into a sentinel-guarded row-strided destination as well"""
    from videoglamm_amd import ops
    x, w = E.ints((M, K), seed=M + K), E.ints((N, K), seed=N + K)
    bias, _, res = E.epilogue_operands(M, N, K)
    a2 = E.ints((M // 3, K), seed=5)
    xd, wd, bd = x.to(cuda, BF), w.to(cuda, BF), bias.to(cuda)
    x_add = x + a2.repeat(3, 1)
    forms = [("plain", dict(), x, E.reference(x, w, bias, out_dtype=BF)),
             ("relu", dict(act=ops.ACT_RELU), x, E.reference(x, w, bias, relu=True, out_dtype=BF)),
             ("residual", dict(residual=res.to(cuda)), x, E.reference(x, w, bias, residual=res, out_dtype=BF)),
             ("A + A2", dict(add=a2.to(cuda, BF)), x_add, E.reference(x_add, w, bias, out_dtype=BF))]
    for name, kw, xe, want in forms:
        what = f"linear_rows {name} M={M} N={N} K={K}"
        E.check(ops.linear_rows(xd, wd, bd, **kw), want, xe, w, what)
        big, view = E.sentinel_out(M, N, BF, cuda)
        ops.linear_rows(xd, wd, bd, out=view, **kw)
        E.check(view, want, xe, w, what + " (strided out)")
        assert E.sentinel_intact(big, M, N), what + ": written outside [M, N]"
    rows = M // 3
    blk = torch.full((3, rows + 40, K), E.POISON, dtype=BF, device=cuda)
    blk[:, 24:24 + rows] = xd.view(3, rows, K)
    wb = E.poisoned(w, dtype=BF).to(cuda)[:N, :K]
    y = ops.linear_rows(blk[:, 24:24 + rows], wb, bd, residual=res.view(3, rows, N).to(cuda))
    E.check(y, E.reference(x, w, bias, residual=res, out_dtype=BF).view(3, rows, N), x, w, f"linear_rows block-strided A M={M} N={N} K={K}")
