"""vg_spatial.hip, the element-wise kernels of vg_pointwise.hip and vg_heads_blockdiag on every route and past the grid cap (-m gpu).

These kernels had one or two small shapes each in tests/test_kernels_gpu.py at tol(dtype) = 2e-2, none past one grid-stride pass (sp_grid / pw_grid cap the
grid at 4096 workgroups = 1,048,576 work items, vg_heads_blockdiag at 2048), and several routes no test selected.  Here (tests/_layout_ref.py: the designs,
the float64 references and the wrong kernels; tests/test_layout_selfcheck.py: each wrong kernel fails on the CPU) operands are small integers, so the output
must equal the float64 statement rounded once: torch.equal, no tolerance.  Every entry point is called directly with an output inside a sentinel-filled
buffer (64 guard elements on each side must stay untouched).  "past one pass": a case whose work-item count, as its launcher counts, lies between
1,048,577 and 1.1 M and is no multiple of 256; the largest ones are compared on the head and the tail of the leading output dimension (the tail is what
the second pass writes), the sentinels around them always.

Per entry point: the routes and geometries run (>> marks what no test ran before), and what is left out.
  vg_permute5        >> the model's gather (B, H, W, 3, 1) with strides (3HW, W, 1, HW, 0), a size-1 dim of stride 0, at C = 3; >> a true 5-D permutation
                     with all dims > 1; >> a dim of size 0 (returns without a launch); bf16 and fp32; >> past one pass: B 2, 420 x 420, both dtypes.
  vg_im2col          >> C 3, 7x7 stride 4 pad 3, Kpad 160 (13 x 9: every border tap and the zero tail; >> past one pass at 324 x 324); >> C 3, k = stride = 14,
                     pad 0 (29 x 43); C 16, 3x3 stride 2 pad 1, Kpad 160 (7 x 5); bf16 and fp32; every input pixel a non-zero integer.
  vg_dwconv          strip kernel (bf16, k 7, C % 8 == 0): W in {1, 3, 4, 5, 7, 9} x H in {1, 4, 7} (the 4-pixel strip tail and all four borders inside the
                     7-tap reach), >> past one pass as 2731 x 3 x 5 x 512 (B H ceil(W / 4) C / 8 items, head and tail batches compared); scalar kernel: fp32
                     and >> bf16 with C = 12, k in {3, 5, 7}, >> past one pass in both dtypes; >> the strip kernel against the scalar kernel on random
                     bf16 data at C = 8, bit for bit (the scalar kernel reached through a weight pointer that is not 16-byte aligned).
  vg_pixel_shuffle2, vg_upsample2_add   with and without bias, bf16 and fp32, >> past one pass (181 x 182, C 8).
  vg_pool2           max and avg (avg on multiples of 4) on the scalar and the vec8 route, contiguous and >> with a pixel stride ([..., a:b] of a fused
                     tensor), >> the misaligned bf16 view that falls back to the scalar route, >> each route past one pass.
  vg_window_partition / vg_window_unpartition   >> the scalar route (bf16 C in {4, 12}, fp32 C in {1, 3}) and the 16-byte chunk route (C 8), ws in
                     {4, 7, 8} with H and W no multiples of ws (and one that is); padding tokens exactly 0; unpartition of windows whose padding tokens
                     hold garbage gives the image back; >> both routes past one pass in both directions.
  vg_bilinear / vg_bilinear_mask   scales 2, 4 and 1/2 with integer logits: vg_bilinear equals the float64 statement bit for bit and vg_bilinear_mask
                     equals ref64 > 0; more than 2 % of the outputs are exactly 0 (the strict > 0); Wo % 4 != 0 (byte stores), Ho % 4 != 0 (last row
                     group); >> Wi = 2048 on the rows kernel (64 KB of dynamic LDS + 32 static bytes: the launcher now raises the limit, see DESIGN.md
                     section 2); >> Wi = 2052 on bilinear_mask_kernel, the fallback, with word and byte stores, >> and past one pass; vg_bilinear past one pass.
  vg_conv3s2_ln_gelu integer x and w (exact sums); LayerNorm + GELU against float64 at rounding level through _rowwise_ref (unit = 1.13 x the LayerNorm unit
                     + the GELU unit and fixed term; multiple from the CPU fp32 statement x 4, floor 4); both channel pairs, both dtypes, 1x1, 7x9, 2x2,
                     12x31; >> past one pass: 1 -> 4 at 2050 x 2050 (bf16) and 4 -> 16 as 4113 x 30 x 34 (fp32).
  vg_axpby           >> past the cap on the scalar route, the vec route with bf16 b, with fp32 b, and with a broadcast b_period (integers: exact).
  vg_activation (ReLU exact; erf GELU tail = head), vg_swiglu (tail = head), vg_cast, vg_where_rows (with ld_out), vg_mask_for_mem (binarize exact;
                     sigmoid tail = head), vg_threshold, vg_embed: >> each just past 1,048,576 items.  "tail = head": the input past the first pass repeats a
                     stretch of the head (not the stretch a loop that re-ran the first pass's items would read), the output is prefilled with NaN inside its guard,
                     and its tail must be bit-equal to that stretch of its head.
  vg_heads_blockdiag and its gather   exact against tests/_cpu_ops.py, nt in {1, 7, 9, 16} x TP in {8, 16}, bf16 and fp32; >> over 2048 x 256 items: N 33,
                     TP 16 and the gather at N 461, nt 9 (the scatter's count is always a multiple of 256: only the gather's second pass is ragged).
Left out: the rows kernel of vg_bilinear_mask has no grid cap (a workgroup per 4 output rows); rope / norm kernels of vg_pointwise.hip and vg_rowops.hip
(tests/test_rowwise_accuracy_gpu.py); shapes past 2^31 elements (the kernels index in int64; the largest case here has 50 M elements).

Measured on the MI355X (also DESIGN.md section 2): all 156 exact cases pass (torch.equal, guards intact), among them every past-one-pass case and Wi = 2048
on the rows kernel after the launcher's fix; the strip dwconv kernel equals the scalar kernel bit for bit on the four random shapes; conv3s2_ln_gelu over its
18 cases: the kernel needed 0.84 units, the CPU fp32 statement 1.32, allowed 4 - 5.3, mismatch share 0 (statement 7e-6).  The 45 tests of this file take 5 s;
the slowest cases: conv3s2 1 -> 4 at 2050 x 2050 0.7 s, pool2 vec8 of a 50 M element fused tensor 0.5 s.
Finding: vg_bilinear_mask at Wi = 2048 asked for 64 KB of dynamic LDS plus 32 static bytes without raising the kernel's limit (fixed in the launcher).
"""
import ctypes

import pytest
import torch

import _layout_ref as L
import _rowwise_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BF, F32 = L.BF, L.F32
GUARD = 64


def _api():
    from videoglamm_amd import _lib, ops
    return _lib.load(), _lib, ops


def _guarded(shape, dtype, cuda):
    """a sentinel-filled buffer and the contiguous view of `shape` inside it (GUARD elements on each side; the view is 64-byte aligned)"""
    n = 1
    for s in shape:
        n *= s
    big = torch.full((n + 2 * GUARD,), L.SENT, dtype=dtype, device=cuda)
    return big, big[GUARD:GUARD + n].view(shape)


def _intact(big):
    return bool((big[:GUARD] == L.SENT).all()) and bool((big[-GUARD:] == L.SENT).all())


def _run(case, cuda):
    """calls the case's entry point with a guarded output; -> (the whole output on the device, the guard is intact)"""
    lib, _lib, ops = _api()
    c, p, st = case.call, ops._p, ops._stream()
    d = lambda t: None if t is None else t.to(cuda)          # noqa: E731
    big, out = _guarded(case.out_shape, case.out_dtype, cuda)
    r = case.route
    if r == "permute5_kernel":
        x = d(c["x"])
        rc = lib.vg_permute5(p(x), p(out), (ctypes.c_int64 * 5)(*c["dims"]), (ctypes.c_int64 * 5)(*c["strides"]), ops._dt(x), st)
    elif r == "im2col_kernel":
        x = d(c["x"])
        B, H, W, C = x.shape
        rc = lib.vg_im2col(p(x), p(out), B, H, W, C, c["k"], c["k"], c["stride"], c["pad"], c["kpad"], ops._dt(x), st)
    elif r.startswith("dwconv"):
        x, w, b = d(c["x"]), d(c["w"]), d(c["bias"])
        B, H, W, C = x.shape
        rc = lib.vg_dwconv(p(x), p(w), p(b), p(out), B, H, W, C, c["k"], ops._dt(x), st)
    elif r.startswith("conv3s2"):
        x, w, b, lw, lb = (d(c[k]) for k in ("x", "w", "bias", "lw", "lb"))
        B, H, W, Cin = x.shape
        rc = lib.vg_conv3s2_ln_gelu(p(x), p(w), w.stride(0), p(b), p(lw), p(lb), c["eps"], p(out), B, H, W, Cin, w.shape[0], ops._dt(x), st)
    elif r == "pixel_shuffle2_kernel":
        g, b = d(c["g"]), d(c["bias"])
        rc = lib.vg_pixel_shuffle2(p(g), p(b), p(out), c["B"], c["H"], c["W"], c["C"], ops._dt(g), st)
    elif r == "upsample2_add_kernel":
        lat, top = d(c["lat"]), d(c["top"])
        B, H, W, C = top.shape
        rc = lib.vg_upsample2_add(p(lat), p(top), p(out), B, H, W, C, ops._dt(top), st)
    elif r.startswith("pool2"):
        fused = d(c["fused"])
        x = fused[..., c["c0"]:c["c0"] + c["C"]]
        B, H, W, C = x.shape
        rc = lib.vg_pool2(p(x), p(out), B, H, W, C, x.stride(2), int(c["is_max"]), ops._dt(x), st)
    elif r.startswith("window_part_kernel reverse"):
        win = d(c["win"])
        rc = lib.vg_window_unpartition(p(win), p(out), c["B"], c["H"], c["W"], win.shape[-1], c["ws"], ops._dt(win), st)
    elif r.startswith("window_part_kernel"):
        x = d(c["x"])
        B, H, W, C = x.shape
        rc = lib.vg_window_partition(p(x), p(out), B, H, W, C, c["ws"], ops._dt(x), st)
    elif r.startswith("bilinear"):
        x = d(c["x"])
        N, Hi, Wi = x.shape
        fn = lib.vg_bilinear if r == "bilinear_kernel" else lib.vg_bilinear_mask
        rc = fn(p(x), p(out), N, Hi, Wi, c["Ho"], c["Wo"], st)
    elif r == "heads_bd_kernel":
        x = d(c["x"])
        rc = lib.vg_heads_blockdiag(p(x), p(out), x.shape[0], x.shape[1], c["TP"], 0, ops._dt(x), st)
    elif r == "heads_bd_gather_kernel":
        x = d(c["full"])
        rc = lib.vg_heads_blockdiag(p(x), p(out), c["N"], c["nt"], c["TP"], 1, ops._dt(x), st)
    else:
        raise AssertionError(r)
    _lib.check(rc, case.name)
    torch.cuda.synchronize()
    return out, _intact(big)


FAMILIES = dict(permute5=L.permute5_cases, im2col=L.im2col_cases, dwconv=L.dwconv_cases, shuffle=L.shuffle_cases, pool2=L.pool2_cases, window=L.window_cases,
                bilinear=L.bilinear_cases, heads=L.heads_cases)
_PARAMS = [(f, False) for f in FAMILIES] + [(f, i) for f in FAMILIES for i in range(L.N_BIG[f])]
_ID = lambda v: v if isinstance(v, str) else ("small" if v is False else f"past{v}")          # noqa: E731


@pytest.mark.parametrize("family,big", _PARAMS, ids=_ID)
def test_exact(cuda, family, big):
    cases = FAMILIES[family](big)
    assert cases
    for case in cases:
        if big is not False:
            assert case.past() and (L.past_one_pass(case.n_items, case.cap) or case.route == "heads_bd_kernel"), (case.name, case.n_items)
        out, intact = _run(case, cuda)
        band = case.band(out).cpu()
        print(f"EXACT {case.name:70s} route {case.route:34s} items {case.n_items}")
        L.equal(case, band)
        assert intact, f"{case.name}: a write outside the output"


def test_routes_named(cuda):
    """every route of the docstring is selected by a small case (the routes are restated from the launchers: the library has no query for them)"""
    routes = {c.route for f in FAMILIES.values() for c in f(False)}
    assert routes >= {"permute5_kernel", "im2col_kernel", "dwconv_kernel", "dwconv_strip_kernel<7>", "pixel_shuffle2_kernel", "upsample2_add_kernel", "pool2_kernel",
                      "pool2_vec8_kernel", "window_part_kernel scalar", "window_part_kernel chunk", "window_part_kernel reverse scalar",
                      "window_part_kernel reverse chunk", "bilinear_kernel", "bilinear_mask_rows_kernel", "bilinear_mask_kernel", "heads_bd_kernel",
                      "heads_bd_gather_kernel"}, routes
    wi = {c.call["x"].shape[2] for f in (L.bilinear_cases,) for c in f(False) if c.route.startswith("bilinear_mask")}
    assert {2048, 2052} <= wi


def test_permute5_empty(cuda):
    """a dim of size 0: returns without a launch and writes nothing"""
    lib, _lib, ops = _api()
    x = torch.ones(8, dtype=BF, device=cuda)
    big, out = _guarded((8,), BF, cuda)
    rc = lib.vg_permute5(ops._p(x), ops._p(out), (ctypes.c_int64 * 5)(2, 0, 3, 1, 1), (ctypes.c_int64 * 5)(1, 1, 1, 1, 1), ops._dt(x), ops._stream())
    _lib.check(rc, "vg_permute5")
    torch.cuda.synchronize()
    assert bool((big == L.SENT).all())


@pytest.mark.parametrize("B,H,W", [(2, 7, 9), (1, 1, 1), (1, 4, 5), (3, 9, 4)])
def test_dwconv_strip_equals_scalar(cuda, B, H, W):
    """the strip kernel's comment claims bit-for-bit agreement with the scalar kernel: random (non-integer) bf16 data at C = 8, the scalar kernel
    reached with the same operands through a weight pointer 4 bytes off a 16-byte boundary (the route rule of vg_dwconv)"""
    lib, _lib, ops = _api()
    x, w, b = (t.to(cuda) for t in L.dwconv_random(B, H, W, seed=H * W))
    wbuf = torch.zeros(w.numel() + 4, dtype=F32, device=cuda)
    w_off = wbuf[1:1 + w.numel()].view(w.shape)
    w_off.copy_(w)
    assert w.data_ptr() % 16 == 0 and w_off.data_ptr() % 16 == 4
    outs = []
    for wt in (w, w_off):
        big, out = _guarded(x.shape, BF, cuda)
        _lib.check(lib.vg_dwconv(ops._p(x), ops._p(wt), ops._p(b), ops._p(out), B, H, W, 8, 7, ops._dt(x), ops._stream()), "vg_dwconv")
        torch.cuda.synchronize()
        assert _intact(big)
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]), f"{int((outs[0] != outs[1]).sum())} of {outs[0].numel()} elements differ between the strip and the scalar kernel"
    import _cpu_ops
    ref = _cpu_ops.dwconv(x.cpu(), w.cpu(), b.cpu(), 7).float()
    assert float((outs[0].cpu().float() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())          # (one bf16 rounding of an O(max) value: sanity only)


@pytest.mark.parametrize("big", [False] + list(range(L.N_BIG["conv3s2"])), ids=_ID)
def test_conv3s2_ln_gelu(cuda, big):
    for ex, case in L.conv3s2_cases(big):
        if big is not False:
            assert ex.past() and L.past_one_pass(ex.n_items)
        out, intact = _run(ex, cuda)
        R.check(case, ex.band(out).cpu().reshape(case.refs[0].shape))
        assert intact, ex.name


# ------------------------------------------------------------------ vg_pointwise.hip past the cap
def _call(name, *args):
    lib, _lib, ops = _api()
    _lib.check(getattr(lib, name)(*args, ops._stream()), name)
    torch.cuda.synchronize()


@pytest.mark.parametrize("route", ["scalar fp32", "scalar ragged bf16", "vec bf16 b", "vec fp32 b", "vec broadcast b_period"])
def test_axpby_past_cap(cuda, route):
    """2 a - 3 b on integers (exact) just past one pass of each route; the vec routes count 8 elements per item"""
    lib, _lib, ops = _api()
    vec = route.startswith("vec")
    n = L.pointwise_n(8 if vec else 1) + (0 if vec or route == "scalar fp32" else 3)          # (n % 8 != 0 keeps a bf16 pair on the scalar route)
    adt = F32 if route == "scalar fp32" else BF
    bdt = F32 if route in ("scalar fp32", "vec fp32 b") else BF
    period = 4096 if route == "vec broadcast b_period" else n
    a = L.ints((n,), (-3, -2, -1, 1, 2, 3), 1).to(adt)
    b = L.ints((period,), (-5, -2, 1, 4), 2).to(bdt)
    assert (adt == BF and n % 8 == 0 and period % 8 == 0) == vec
    want = L.once(2.0 * a.double() - 3.0 * b.double().repeat(-(-n // period))[:n], adt)
    big, out = _guarded((n,), adt, cuda)
    ga, gb = a.to(cuda), b.to(cuda)
    _call("vg_axpby", ops._p(ga), ops._p(gb), ops._p(out), n, 2.0, -3.0, period, ops._dt(ga), ops._dt(gb), ops._dt(out))
    assert torch.equal(out.cpu(), want) and _intact(big)


def test_activation_past_cap(cuda):
    lib, _lib, ops = _api()
    n = L.pointwise_n(1)
    x = L.ints((n,), (-3, -2, -1, 1, 2, 3), 3).to(BF)
    big, out = _guarded((n,), BF, cuda)
    gx = x.to(cuda)
    _call("vg_activation", ops._p(gx), ops._p(out), n, R.ACT_RELU, ops._dt(gx), ops._dt(out))
    assert torch.equal(out.cpu(), x.clamp_min(0)) and _intact(big)
    src, _ = L.repeat_tail(n)
    for dt in (BF, F32):
        x = (3.0 * torch.randn(n, generator=torch.Generator().manual_seed(4)))[src].to(dt)
        big, out = _guarded((n,), dt, cuda)
        out.fill_(float("nan"))
        gx = x.to(cuda)
        _call("vg_activation", ops._p(gx), ops._p(out), n, R.ACT_GELU, ops._dt(gx), ops._dt(out))
        assert L.tail_equals_head(out, n) and _intact(big)
        assert float((out.cpu().float() - torch.nn.functional.gelu(x.float())).abs().max()) < 0.05          # (it is a GELU: the accuracy is test_rowwise_accuracy_gpu's)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_swiglu_past_cap(cuda, dt):
    lib, _lib, ops = _api()
    Fh = 37
    M = -(-L.pointwise_n(1) // Fh)
    n = M * Fh
    assert L.past_one_pass(n)
    src, _ = L.repeat_tail(n)
    g = torch.Generator().manual_seed(5)
    gate, up = (2.0 * torch.randn(n, generator=g))[src].view(M, Fh), torch.randn(n, generator=g)[src].view(M, Fh)
    gu = torch.cat([gate, up], dim=1).to(dt).to(cuda)
    big, out = _guarded((M, Fh), dt, cuda)
    out.fill_(float("nan"))
    _call("vg_swiglu", ops._p(gu), ops._p(out), M, Fh, ops._dt(gu))
    assert L.tail_equals_head(out, n) and _intact(big)
    import _cpu_ops
    assert torch.allclose(out.cpu().float(), _cpu_ops.swiglu(gu.cpu()).float(), rtol=2e-2, atol=2e-2)          # (it is a SwiGLU: the accuracy is test_rowwise_accuracy_gpu's)


def test_cast_threshold_mask_past_cap(cuda):
    lib, _lib, ops = _api()
    n = L.pointwise_n(1)
    x = L.ints((n,), (-3.5, -1.0, 0.0, 0.0, 0.40625, 2.0), 6)          # bf16-exact values with zeros: the strict > 0
    gx = x.to(cuda)
    big, out = _guarded((n,), BF, cuda)
    _call("vg_cast", ops._p(gx), ops._p(out), n, ops._dt(gx), ops._dt(out))
    assert torch.equal(out.cpu(), x.to(BF)) and _intact(big)
    big, out = _guarded((n,), torch.uint8, cuda)
    _call("vg_threshold", ops._p(gx), ops._p(out), n)
    assert torch.equal(out.cpu(), (x > 0).to(torch.uint8)) and _intact(big)
    big, out = _guarded((n,), BF, cuda)
    _call("vg_mask_for_mem", ops._p(gx), ops._p(out), n, 1, 20.0, -10.0, ops._dt(out))
    assert torch.equal(out.cpu(), ((x > 0).float() * 20.0 - 10.0).to(BF)) and _intact(big)
    src, _ = L.repeat_tail(n)
    xs = (4.0 * torch.randn(n, generator=torch.Generator().manual_seed(7)))[src].to(cuda)
    big, out = _guarded((n,), F32, cuda)
    out.fill_(float("nan"))
    _call("vg_mask_for_mem", ops._p(xs), ops._p(out), n, 0, 20.0, -10.0, ops._dt(out))
    assert L.tail_equals_head(out, n) and _intact(big)
    assert float((out.cpu() - (torch.sigmoid(xs.cpu()) * 20.0 - 10.0)).abs().max()) < 1e-4


def test_where_rows_past_cap(cuda):
    """rows of 37 elements written at a row stride of 40 (ld_out): the gap columns keep the sentinel"""
    lib, _lib, ops = _api()
    inner, ld = 37, 40
    rows = -(-L.pointwise_n(1) // inner)
    assert L.past_one_pass(rows * inner)
    a = L.ints((rows, inner), (-3, -2, -1, 1, 2, 3), 8).to(BF)
    b = L.ints((inner,), (-6, -5, 5, 6), 9).to(BF)
    cond = L.ints((rows,), (-1.0, 0.0, 1.0, 2.0), 10)
    big, out = _guarded((rows, ld), BF, cuda)
    ga, gb, gc = a.to(cuda), b.to(cuda), cond.to(cuda)
    _call("vg_where_rows", ops._p(gc), ops._p(ga), ops._p(gb), ops._p(out), rows, inner, inner, 0.0, ld, ops._dt(ga))
    o = out.cpu()
    assert torch.equal(o[:, :inner], torch.where(cond[:, None] > 0, a, b[None, :].expand_as(a)))
    assert bool((o[:, inner:] == L.SENT).all()) and _intact(big)


def test_embed_past_cap(cuda):
    lib, _lib, ops = _api()
    D = 24
    n = -(-L.pointwise_n(1) // D)
    assert L.past_one_pass(n * D)
    table = L.ints((97, D), (-3, -2, -1, 1, 2, 3), 11).to(BF)
    ids = torch.randint(0, 97, (n,), generator=torch.Generator().manual_seed(12))
    ids[-3:] = torch.tensor([96, 0, 95])
    big, out = _guarded((n, D), BF, cuda)
    gt, gi = table.to(cuda), ids.to(cuda)
    _call("vg_embed", ops._p(gi), ops._p(gt), ops._p(out), n, D, ops._dt(gt))
    assert torch.equal(out.cpu(), table[ids]) and _intact(big)
