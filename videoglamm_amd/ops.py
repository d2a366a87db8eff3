"""Host-side operator layer: torch tensors in, C-ABI calls (include/vg_kernels.h) out.

PyTorch is used for device memory and streams only; every arithmetic op on the VideoGLaMM hot path
goes through a hand-written gfx950 kernel in libvgkernels.so.  All tensors are token-major
(channels last).  There is no CPU fallback: calling any op with a CPU tensor raises.
"""
import ctypes

import torch

from . import _lib

F32, BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_SILU, ACT_SIGMOID = 0, 1, 2, 3, 4, 5


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def _tdt(code):
    return torch.float32 if code == F32 else torch.bfloat16


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.VGKernelError("VideoGLaMM ops run on the MI355X HIP kernels only; got a CPU tensor")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


import contextlib as _contextlib


_capture_lock = __import__("threading").Lock()
_capture_depth = [0, True]      # [captures in flight, the collector was enabled when the first one began]


@_contextlib.contextmanager
def graph_capture(g):
    """torch.cuda.graph(g) with Python's cyclic garbage collector held off for the duration of the capture.  A capture of the decode step or of
    the SAM2 propagation creates tens of thousands of Python objects, so a generation-2 collection WILL run inside it in a long-lived process —
    and if that collection finalises device objects of an earlier clip that sit in reference cycles (an evicted CUDAGraph, events), the runtime
    calls their destructors make are illegal while a stream is capturing and abort the process (seen r03: tests/test_kernels_gpu.py's graph
    tests followed by an end-to-end capture in one process)."""
    import gc
    # the collector is process-wide state: a lock + depth counter make nested / concurrent captures restore it exactly once
    with _capture_lock:
        if _capture_depth[0] == 0:
            gc.collect()
            _capture_depth[1] = gc.isenabled()
            gc.disable()
        _capture_depth[0] += 1
    try:
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            yield
    finally:
        with _capture_lock:
            _capture_depth[0] -= 1
            if _capture_depth[0] == 0 and _capture_depth[1]:
                gc.enable()


def graph_node_counts(g):
    """(kernel nodes, memcpy nodes, other nodes) of a torch.cuda.CUDAGraph created with keep_graph=True: launches per replay, read off the
    captured hipGraph_t itself (vg_graph_node_counts)."""
    import ctypes
    counts = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().vg_graph_node_counts(ctypes.c_void_p(int(g.raw_cuda_graph())), counts), "vg_graph_node_counts")
    return tuple(int(c) for c in counts)


def _f32(t):
    if t is None:
        return None
    assert t.dtype == torch.float32 and t.is_contiguous(), "bias/gamma/norm vectors are fp32 contiguous"
    return t


def _rows2d(x):
    """View x[..., K] as 2-D [M, K] with a single row stride (no copy when possible)."""
    K = x.shape[-1]
    if x.dim() == 2 and x.stride(1) == 1:
        return x, x.shape[0], x.stride(0) if x.shape[0] > 1 else max(x.stride(0), K)
    if not x.is_contiguous():
        x = x.contiguous()
    x2 = x.view(-1, K)
    return x2, x2.shape[0], K


def _splitk(M, N, K, es):
    """K slices for a GEMM whose 128x128 tiles leave most of the 256 CUs (two workgroups each) idle while K is long:
    measured r01 (tools/bench_gemm.py): the Llama down projection at M = 213 streams 117 MB of weights in 157 us on 64 tiles."""
    import os
    if M <= 16 or N % 8 or os.environ.get("VG_GEMM_SPLITK", "1") == "0":
        return 0
    tiles = -(-M // 128) * -(-N // 128)
    steps = K * es // 128
    if tiles > int(os.environ.get("VG_GEMM_SPLITK_TILES", "256")) or steps < 32:
        return 0
    ks = min(8, 512 // tiles, steps // 16)
    return ks if ks >= 2 else 0


def _linear_splitk(lib, x, x2, M, lda, w, bias, act, gamma, residual, odt, ks, out=None):
    N, K = w.shape
    y = out if out is not None else torch.empty(*x.shape[:-1], N, dtype=odt, device=x.device)
    assert y.numel() == M * N
    ws = torch.empty(ks * M * N, dtype=torch.float32, device=x.device)
    r2, ldr = None, 0
    if residual is not None:
        r2, mr, ldr = _rows2d(residual)
        assert mr == M and r2.shape[1] == N and r2.dtype == odt
    rc = lib.vg_gemm_splitk(_p(x2), lda, _p(w), w.stride(0), _p(y), N, _p(_f32(bias)), _p(_f32(gamma)), _p(r2), ldr, M, N, K, _dt(x2), _dt(y),
                            int(act), ks, _p(ws), ws.numel(), _stream())
    _lib.check(rc, "vg_gemm_splitk")
    return y


import os as _os
_TAILSPLIT = True


def linear(x, w, bias=None, act=ACT_NONE, gamma=None, residual=None, out_dtype=None, out=None, glu=False):
    """y[..., N] = ((act(x @ w^T + bias)) * gamma) + residual ; w: [N, K] (row stride may exceed K).
    glu: w is [2N, K] = gate rows | up rows and y = silu(x @ gate^T) * (x @ up^T) — done in the GEMV epilogue for
    <= 16 rows (decode), as GEMM + vg_swiglu otherwise."""
    return _linear(x, w, bias, act, gamma, residual, out_dtype, out, glu)


def _linear(x, w, bias=None, act=ACT_NONE, gamma=None, residual=None, out_dtype=None, out=None, glu=False):
    lib = _lib.load()
    if glu and x.numel() // x.shape[-1] > 16 and ((w.shape[0] // 2) % 8 != 0 or residual is not None or gamma is not None
                                                  or (out is not None and not (out.is_contiguous() and out.data_ptr() % 16 == 0))):
        return swiglu(_linear(x, w, bias))     # shapes the fused epilogue does not take (odd widths)
    x2, M, lda = _rows2d(x)
    N, K = w.shape
    if glu:
        N //= 2
    assert x2.shape[1] == K, (x.shape, w.shape)
    assert w.stride(1) == 1
    odt = out_dtype if out_dtype is not None else x.dtype
    # a few rows past a multiple of 256 (the C2 prompt: 3361 = 13 x 256 + 33) cost the 256x256-tile kernel a whole extra row of tiles;
    # when dropping that row of tiles saves a ROUND of 256 workgroups, the tail rows go through their own (128-tile / skinny) launch:
    # Llama gate|up at M = 3361: 1568 tiles = 7 rounds -> 1456 tiles = 6 rounds + a 33-row launch
    rem = M % 256
    if (_TAILSPLIT and M > 1024 and 0 < rem <= 64 and x2.dtype == torch.bfloat16 and x2.is_contiguous() and (out is None or out.is_contiguous())
            and lib.vg_gemm_route(M, N, K, BF16, 1 if glu else 0, 0) == 3):
        ntw = -(-N // (128 if glu else 256))
        if -(-((M // 256) * ntw) // 256) < -(-((M // 256 + 1) * ntw) // 256):
            M0 = M - rem
            y = out if out is not None else torch.empty(*x.shape[:-1], N, dtype=odt, device=x.device)
            y2 = y.view(M, N)
            r2 = None if residual is None else residual.reshape(M, N)
            for a, b_ in ((0, M0), (M0, M)):
                _linear(x2[a:b_], w, bias, act, gamma, None if r2 is None else r2[a:b_], out_dtype, y2[a:b_], glu)
            return y
    if (out is not None and out.dim() == 3 and not out.is_contiguous() and out.stride(2) == 1 and x.dim() == 3 and x.is_contiguous()
            and residual is None and not glu and out.shape[:2] == x.shape[:2]):
        # [B, rows, N] rows of a larger buffer (the memory bank's slot of each object): one batched launch, batch stride = out.stride(0)
        B, Mb = x.shape[0], x.shape[1]
        assert out.dtype == odt and out.shape[2] == N and _dt(w) == _dt(x)
        rc = lib.vg_gemm(_p(x), K, Mb * K, _p(w), w.stride(0), 0, _p(out), out.stride(1), out.stride(0), _p(_f32(bias)), _p(_f32(gamma)),
                         None, 0, 0, Mb, N, K, B, _dt(x), _dt(out), act, 0, _stream())
        _lib.check(rc, "vg_gemm(batched rows)")
        return out
    ks = _splitk(M, N, K, x2.element_size()) if (not glu and (out is None or (out.is_contiguous() and out.dtype == odt))) else 0
    if ks:
        return _linear_splitk(lib, x, x2, M, lda, w, bias, act, gamma, residual, odt, ks, out)
    if out is None:
        out = torch.empty(*x.shape[:-1], N, dtype=odt, device=x.device)
    o2, Mo, ldc = _rows2d(out)
    assert Mo == M and out.dtype == odt and out.shape[-1] == N, (tuple(out.shape), M, N, out.dtype, odt)      # (a wider / narrower `out` would be written with a wrong row stride)
    assert o2.data_ptr() == out.data_ptr() and (o2.is_contiguous() or out.dim() == 2), "out must be contiguous or a 2-D row-strided view"
    r2, ldr = None, 0
    if residual is not None:
        assert residual.dtype == odt
        r2, Mr, ldr = _rows2d(residual)
        assert Mr == M and r2.shape[1] == N
    assert _dt(w) == _dt(x2)
    rc = lib.vg_gemm(_p(x2), lda, 0, _p(w), w.stride(0), 0, _p(o2), ldc, 0, _p(_f32(bias)), _p(_f32(gamma)),
                     _p(r2), ldr, 0, M, N, K, 1, _dt(x2), _dt(out), act, int(bool(glu)), _stream())
    _lib.check(rc, "vg_gemm")
    return out


def linear_rows(x, w, bias=None, act=ACT_NONE, residual=None, out=None, ln=None, add=None, rope=None, force_fused=False):
    """y = act(pro(x) @ w^T + bias) [RoPE] [+ residual] on short rows, ONE launch in bf16 (vg_gemm_rows) while the problem is small — the fp32 parity
    mode, shapes the kernel does not take and large row counts (see below; force_fused overrides) run the same arithmetic as the separate launches.
    ln = (weight, bias, eps): LayerNorm over the last dim first;  add = a2 [rows2, K]: x + a2, a2 repeated over blocks of rows2 rows;
    rope = (cos, sin, cols, ch, rows_per_block, r0, r1, grid): axial RoPE (rope_axial_heads_) on the first `cols` output columns, heads of `ch`
    channels, rows [r0, r1) of every block of rows_per_block rows, token = (row - r0) % grid.  out: optional [.., N] destination (row stride free)."""
    lib = _lib.load()
    N, K = w.shape
    sA = 0
    if x.dim() == 3 and x.stride(2) == 1 and not x.is_contiguous() and x.dtype == torch.bfloat16:
        # a strided [B, rows, K] view (the memory bank's valid rows): addressed in place by block stride
        x2, M, lda, sA = x, x.shape[0] * x.shape[1], x.stride(1), x.stride(0)
        assert rope is None or rope[4] == x.shape[1]
    else:
        x2, M, lda = _rows2d(x)
    assert x2.shape[-1] == K and w.stride(1) == 1 and not (ln is not None and add is not None)
    fused = x2.dtype == torch.bfloat16 and K in (64, 128, 192, 256) and N % 64 == 0 and (rope is None or (act == ACT_NONE and residual is None)) \
        and (act == ACT_NONE or residual is None)
    if fused and ln is not None and not force_fused:
        # the 64 x 64-tile kernel pays while the problem is small (every workgroup re-stages W, and the LayerNorm is redone per column group): measured
        # r05 (tools/lab/rows_bench.py, K = 256): norm -> linear -> ReLU at M = 4096: N = 1024 17.9 us fused / 25.5 separate, N = 2048 29.0 / 25.2;
        # M = 32768 (8 objects), N = 2048: 158 / 69; with the RoPE epilogue the separate path has a third launch: M = 8192, N = 768 24.6 / 33.7,
        # M = 32768: 80.5 / 48.5.  (The A + A2 prologue of the memory keys replaces nine launches and always pays.)
        tiles = -(-M // 64) * (N // 64)
        fused = tiles <= 2048 if rope is not None else tiles < 2048
    if not fused:
        h = x
        if ln is not None:
            h = layernorm(x, ln[0], ln[1], ln[2])
        elif add is not None:
            h = axpby(x.reshape(-1, add.shape[0], K), add, 1.0, 1.0).view(x.shape)
        y = _linear(h, w, bias, act, None, residual, None, out if rope is None else None)
        if rope is not None:
            cos, sin, cols, ch, rpb, r0, r1, grid = rope
            heads, B = cols // ch, M // rpb
            yv = y.view(B, rpb, N)
            if y.dtype == torch.bfloat16 and r0 == 0:
                rope_axial_heads_(yv, heads, cos, sin, r1, grid)        # (the first r1 rows of every block, strided heads: one launch)
            else:
                # (parity mode only: the strided head slices go through a contiguous copy — torch plumbing around vg_rope_axial)
                part = yv[:, r0:r1, :cols].reshape(B, r1 - r0, heads, ch).permute(0, 2, 1, 3).reshape(B * heads, r1 - r0, ch).clone(memory_format=torch.contiguous_format)
                rope_axial_(part, cos, sin, r1 - r0, grid)
                yv[:, r0:r1, :cols] = part.view(B, heads, r1 - r0, ch).permute(0, 2, 1, 3).reshape(B, r1 - r0, cols)
            if out is not None:
                out.copy_(y.view(out.shape))
                y = out
        return y
    if out is None:
        out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
    o2, Mo, ldc = _rows2d(out)
    assert o2.data_ptr() == out.data_ptr(), "out must be contiguous or a 2-D row-strided view (anything else would be written through a copy)"
    assert Mo == M and out.dtype == x.dtype and out.shape[-1] == N
    r2, ldr = None, 0
    if residual is not None:
        r2, Mr, ldr = _rows2d(residual)
        assert Mr == M and r2.shape[1] == N and residual.dtype == x.dtype
    lw = lb = a2 = None
    eps, lda2, rows2 = 0.0, 0, 0
    if ln is not None:
        lw, lb, eps = _f32(ln[0]), _f32(ln[1]), float(ln[2])
        assert lw.numel() == K and lb.numel() == K
    if add is not None:
        a2 = add
        assert a2.dim() == 2 and a2.shape[1] == K and a2.stride(1) == 1 and a2.dtype == x.dtype and M % a2.shape[0] == 0
        lda2, rows2 = a2.stride(0), a2.shape[0]
    cs = sn = None
    cols = ch = rpb = r0 = r1 = grid = 0
    if rope is not None:
        cs, sn, cols, ch, rpb, r0, r1, grid = rope
        cs, sn = _f32(cs), _f32(sn)
        assert M % rpb == 0 and cs.shape[1] * 2 == ch and cs.shape[0] >= grid and cs.is_contiguous() and sn.is_contiguous()
    if sA:
        rpb = x.shape[1]
    rc = lib.vg_gemm_rows(_p(x2), lda, _p(w), w.stride(0), _p(o2), ldc, _p(_f32(bias)), _p(r2), ldr, M, N, K, act, _p(lw), _p(lb), eps,
                          _p(a2), lda2, rows2, _p(cs), _p(sn), int(cols), int(ch), int(rpb), int(sA), int(r0), int(r1), int(grid), BF16, _stream())
    _lib.check(rc, "vg_gemm_rows")
    return out


def mlp_rows(x, ln, w1, b1, w2, b2, force=False):
    """y = x + w2 @ gelu(w1 @ LayerNorm(x) + b1) + b2 — a pre-norm MLP block (Hiera's x + mlp(norm2(x))); ONE launch at the narrow bf16 width
    vg_mlp_rows is routed for (C = 144), the separate launches otherwise (wider rows, the fp32 parity mode).  ln = (weight, bias, eps).
    force: run the fused kernel on any width it has an instantiation for (C = 288: correct, measured slower than the three launches)."""
    lib = _lib.load()
    C, H = x.shape[-1], w1.shape[0]
    ok = lib.vg_mlp_rows_supported(C, H) or (force and C in (144, 288) and H % 32 == 0)
    if not (x.dtype == torch.bfloat16 and ok and w1.shape == (H, C) and w2.shape == (C, H)
            and w1.is_contiguous() and w2.is_contiguous()):
        h = linear_ln(x, ln, w1, b1, ACT_GELU)          # (one launch at stage 2's width: vg_gemm_ln; norm + linear otherwise)
        return linear(h, w2, b2, residual=x)
    x2, M, ldx = _rows2d(x)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    rc = lib.vg_mlp_rows(_p(x2), ldx, _p(out), C, _p(_f32(ln[0])), _p(_f32(ln[1])), float(ln[2]), _p(w1), _p(_f32(b1)), _p(w2), _p(_f32(b2)),
                         M, C, H, BF16, _stream())
    _lib.check(rc, "vg_mlp_rows")
    return out


def linear_ln(x, ln, w, bias=None, act=ACT_NONE, window=None):
    """act(LayerNorm(x) @ w^T + bias); ln = (weight, bias, eps).  window = (B, H, W, ws): x is image-order [B,H,W,K] and the output window-order
    [Bw, ws*ws, N] (window_partition behind the norm, as linear_window's gather).  ONE launch where the row-register kernel is built for the shape
    (vg_gemm_ln: bf16, K = 144 / 288, >= 65536 rows — Hiera stages 1 and 2), the norm and the projection as two launches otherwise."""
    lib = _lib.load()
    N, K = w.shape
    x2, M, lda = _rows2d(x)
    if window is not None:
        B, H, W, ws = window
        Bw = B * (-(-H // ws)) * (-(-W // ws))
        M = Bw * ws * ws
    fused = (x.dtype == torch.bfloat16 and x.is_cuda and w.dtype == x.dtype and w.stride(1) == 1 and act in (ACT_NONE, ACT_GELU)
             and lib.vg_gemm_route(M, N, K, BF16, 0, 1 if window is not None else 0) == 7)
    if not fused:
        xn = layernorm(x, ln[0], ln[1], ln[2])
        return linear_window(xn, w, bias, *window, scatter=False, act=act) if window is not None else linear(xn, w, bias, act=act)
    out = torch.empty((Bw, ws * ws, N) if window is not None else x.shape[:-1] + (N,), dtype=x.dtype, device=x.device)
    o2, _, ldc = _rows2d(out)
    wa = window if window is not None else (0, 0, 0, 0)
    rc = lib.vg_gemm_ln(_p(x2), lda, _p(w), w.stride(0), _p(o2), ldc, _p(_f32(bias)), _p(_f32(ln[0])), _p(_f32(ln[1])), float(ln[2]), M, N, K, act,
                        1 if window is not None else 0, wa[0], wa[1], wa[2], wa[3],
                        _p(_zero_row(K, x.dtype, x.device)) if window is not None else None, BF16, _stream())
    if rc == -3:      # VG_ERR_UNSUPPORTED (include/vg_kernels.h)
        # the route query answers for the contiguous, aligned call (and, since it is built on the launcher's plan, knows the kernel's LDS bound); this
        # call's own pointers and strides can still refuse (16-byte aligned output rows): take the two-launch form
        xn = layernorm(x, ln[0], ln[1], ln[2])
        return linear_window(xn, w, bias, *window, scatter=False, act=act) if window is not None else linear(xn, w, bias, act=act)
    _lib.check(rc, "vg_gemm_ln")
    return out


def mlp3_pack(w):
    """[G, out, in] nn.Linear weights -> vg_mlp3_grouped's fragment order [G, ceil(out / 32), in / 16, 64, 8] (lane = 32 * k-half + row; rows past `out` zero)."""
    G, n_out, n_in = w.shape
    T = -(-n_out // 32)
    wp = torch.zeros(G, T * 32, n_in, dtype=w.dtype, device=w.device)
    wp[:, :n_out] = w
    return wp.view(G, T, 32, n_in // 16, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous().view(G, T, n_in // 16, 64, 8)


def mlp3_grouped(x, G, w0, b0, w1, b1, w2, b2, out, sigmoid_mask=0):
    """G three-layer MLP heads in one launch (vg_mlp3_grouped).  x: a bf16 [R, >= G, K] view (head g reads x[:, g, :]); w0, w1, w2: mlp3_pack of the stacked
    [G, Hd, K], [G, Hd, Hd], [G, No, Hd] bf16 weights, b0 / b1 / b2 fp32 [G, Hd] / [G, Hd] / [G, No]; out: a bf16 / fp32 [R, G, >= No] view whose leading No
    columns are written."""
    lib = _lib.load()
    R, K = x.shape[0], x.shape[2]
    Hd, No = b0.shape[1], b2.shape[1]
    assert x.dtype == torch.bfloat16 and x.stride(2) == 1 and out.stride(2) == 1 and x.shape[1] >= G and out.shape[1] >= G and out.shape[2] >= No
    assert w0.shape == (G, -(-Hd // 32), K // 16, 64, 8) and w1.shape == (G, -(-Hd // 32), Hd // 16, 64, 8) and w2.shape == (G, -(-No // 32), Hd // 16, 64, 8)
    assert all(t.is_contiguous() for t in (w0, b0, w1, b1, w2, b2)) and b0.shape == (G, Hd) and b1.shape == (G, Hd) and b2.shape == (G, No)
    rc = lib.vg_mlp3_grouped(_p(x), x.stride(0), x.stride(1), _p(w0), _p(b0), _p(w1), _p(b1), _p(w2), _p(b2), _p(out), out.stride(0), out.stride(1),
                             _dt(out), G, R, K, Hd, No, int(sigmoid_mask), _stream())
    _lib.check(rc, "vg_mlp3_grouped")
    return out


def heads_blockdiag(x, TP):
    """[N, nt, 128] -> block-diagonal [N * 8 * TP, 128]: row (h, t) holds head h's 16 channels of token t, zeros elsewhere (vg_heads_blockdiag)."""
    x = x.contiguous()
    N, nt, C = x.shape
    assert C == 128 and nt <= TP
    out = torch.empty(N * 8 * TP, 128, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().vg_heads_blockdiag(_p(x), _p(out), N, nt, TP, 0, _dt(x), _stream()), "vg_heads_blockdiag")
    return out


def heads_blockdiag_gather(full, N, nt, TP):
    """the inverse read: full [N * 8 * TP, 128] (rows (h, t)) -> [N, nt, 128], head h's channels of token t from row (h, t)."""
    full = full.contiguous()
    assert full.numel() == N * 8 * TP * 128
    out = torch.empty(N, nt, 128, dtype=full.dtype, device=full.device)
    _lib.check(_lib.load().vg_heads_blockdiag(_p(full), _p(out), N, nt, TP, 1, _dt(full), _stream()), "vg_heads_blockdiag")
    return out


_ZROWS = {}


def _zero_row(K, dtype, device):
    key = (dtype, str(device))
    z = _ZROWS.get(key)
    if z is None or z.numel() < K:
        z = _ZROWS[key] = torch.zeros(max(K, 8192), dtype=dtype, device=device)
    return z


def linear_window(x, w, bias, B, H, W, ws, scatter, act=ACT_NONE, gamma=None, residual=None):
    """Hiera's windowed projections with the partition folded into the GEMM (vg_gemm_window).
    scatter=False: x image-order [B,H,W,K] -> window-order [Bw, ws*ws, N]   (window_partition + linear)
    scatter=True : x window-order [Bw, ws*ws, K] -> image-order [B,H,W,N] (+ residual [B,H,W,N])  (linear + unpartition + add)"""
    lib = _lib.load()
    N, K = w.shape
    nH, nW = -(-H // ws), -(-W // ws)
    Bw = B * nH * nW
    x2, Mx, lda = _rows2d(x)
    assert x2.shape[1] == K and w.stride(1) == 1 and _dt(w) == _dt(x2)
    if scatter:
        assert Mx == Bw * ws * ws, (x.shape, B, H, W, ws)
        out = torch.empty(B, H, W, N, dtype=x.dtype, device=x.device)
    else:
        assert Mx == B * H * W, (x.shape, B, H, W)
        assert residual is None
        out = torch.empty(Bw, ws * ws, N, dtype=x.dtype, device=x.device)
    o2, _, ldc = _rows2d(out)
    r2, ldr = None, 0
    if residual is not None:
        assert residual.dtype == out.dtype
        r2, Mr, ldr = _rows2d(residual)
        assert Mr == B * H * W and r2.shape[1] == N
    rc = lib.vg_gemm_window(_p(x2), lda, _p(w), w.stride(0), _p(o2), ldc, _p(_f32(bias)), _p(_f32(gamma)), _p(r2), ldr, N, K,
                            _dt(x2), _dt(out), act, 2 if scatter else 1, B, H, W, ws, _p(_zero_row(K, x.dtype, x.device)), _stream())
    _lib.check(rc, "vg_gemm_window")
    return out


def bmm_nt(a, w, out_dtype=None, shared_a=False):
    """c[b] = a[b] @ w[b]^T ; a: [B,M,K], w: [B,N,K] (or [N,K] shared) -> [B,M,N].  shared_a: a is ONE [M, >= K] matrix for every batch entry (batch
    stride 0; its leading K columns are used — a K-padded weight), w: [B,N,K]."""
    lib = _lib.load()
    a = a.contiguous()
    w = w.contiguous()
    if shared_a:
        assert a.dim() == 2 and w.dim() == 3 and a.shape[1] >= w.shape[2]
        B, (M, lda), K, sA = w.shape[0], a.shape, w.shape[2], 0
    else:
        B, M, K = a.shape
        lda, sA = K, M * K
    N = w.shape[-2]
    sW = 0 if w.dim() == 2 else N * K
    odt = out_dtype if out_dtype is not None else a.dtype
    out = torch.empty(B, M, N, dtype=odt, device=a.device)
    rc = lib.vg_gemm(_p(a), lda, sA, _p(w), K, sW, _p(out), N, M * N, None, None, None, 0, 0, M, N, K, B,
                     _dt(a), _dt(out), ACT_NONE, 0, _stream())
    _lib.check(rc, "vg_gemm(batched)")
    return out


def _causal_code(causal, window):
    """the kernel's mask code: 0 none, 1 causal, c >= 2 causal with a sliding window of c visible keys (own position included)."""
    if not causal:
        assert not window, "a sliding window needs the causal mask"
        return 0
    assert window == 0 or window >= 2, "a window of one key cannot be expressed (and is not attention)"
    return int(window) if window else 1


_SPLIT_WG_D256 = 256   # workgroups the KV split aims for at head dim 256: one 8-wave workgroup per CU (measured r02: 256 beats 384 / 512 / 1024 by 1.2-2.5x, the fp32 partials are the cost)


def attention(q, k, v, scale, causal=False, window=0):
    """q: [B,Sq,Hq,D], k/v: [B,Skv,Hkv,D] (arbitrary batch/token/head strides, D contiguous) -> [B,Sq,Hq,D].
    window > 0 (with causal): every query sees its own position and the window - 1 before it (sliding-window LLMs)."""
    lib = _lib.load()
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    assert q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    out = torch.empty(B, Sq, Hq, D, dtype=q.dtype, device=q.device)
    # few query rows against a long KV range (LLM decode, mask-decoder tokens -> image): split the KV range over
    # workgroups so the chip is filled, merge the partial softmaxes afterwards
    nsplit, ws = 1, None
    blocks = -(-Sq // (128 if q.dtype == torch.bfloat16 else 64)) * Hq * B   # workgroups without splitting
    if Skv >= 512 and blocks < 384:                                           # < 1.5 workgroups per CU: split KV
        nsplit = max(1, min(64, (_SPLIT_WG_D256 if D > 128 else 512) // blocks, Skv // 128))
    if nsplit > 1:
        ws = torch.empty(B * Hq * nsplit * Sq * (D + 2), dtype=torch.float32, device=q.device)
    rc = lib.vg_attention_splitkv(_p(q), _p(k), _p(v), _p(out), B, Hq, Hkv, Sq, Skv, D,
                                  q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                                  v.stride(0), v.stride(1), v.stride(2), out.stride(0), out.stride(1), out.stride(2),
                                  float(scale), _causal_code(causal, window), _dt(q), _p(ws), 0 if ws is None else ws.numel(), nsplit,
                                  None, _stream())
    _lib.check(rc, "vg_attention")
    return out


def attention_dv(q, k, v, scale):
    """softmax(q k^T * scale) v with values of another width than the keys: q [B,Sq,H,D], k [B,Skv,H,D], v [B,Skv,H,DV] -> [B,Sq,H,DV]
    (vg_attention_dv: SAM2's memory cross-attention on the un-projected memory, D = 256, DV = 64)."""
    lib = _lib.load()
    B, Sq, H, D = q.shape
    Skv, DV = k.shape[1], v.shape[3]
    assert k.shape == (B, Skv, H, D) and v.shape[:3] == (B, Skv, H) and q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    if q.dtype != torch.bfloat16:
        # fp32 parity mode: the values zero-padded to the key width through vg_attention (exact fp32 MFMA chain), the first DV columns kept —
        # the same arithmetic; the DV-wide kernel is built for bf16 only (vg_attention.hip: attention_impl)
        vp = torch.zeros(B, Skv, H, D, dtype=q.dtype, device=q.device)
        vp[..., :DV].copy_(v)
        return attention(q, k, vp, scale)[..., :DV].contiguous()
    out = torch.empty(B, Sq, H, DV, dtype=q.dtype, device=q.device)
    nsplit, ws = 1, None
    # r06: the LDS-DMA form (vg_attention_dma.hip) takes D = 256 / DV = 64 with 256-row query tiles; attn_kernel's key-split form has 128-row tiles
    dma = D == 256 and DV == 64 and Sq >= 256 and q.dtype == torch.bfloat16 and _os.environ.get("VG_ATTN_DMA", "1") != "0"
    blocks = -(-Sq // (256 if dma else 128)) * H * B
    if Skv >= 512 and blocks < 384:
        nsplit = max(1, min(64, _SPLIT_WG_D256 // blocks, Skv // 128))
    if nsplit > 1:
        ws = torch.empty(B * H * nsplit * Sq * (DV + 2), dtype=torch.float32, device=q.device)
    rc = lib.vg_attention_dv(_p(q), _p(k), _p(v), _p(out), B, H, Sq, Skv, D, DV,
                             q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                             v.stride(0), v.stride(1), v.stride(2), out.stride(0), out.stride(1), out.stride(2),
                             float(scale), _dt(q), _p(ws), 0 if ws is None else ws.numel(), nsplit, _stream())
    _lib.check(rc, "vg_attention_dv")
    return out


_WIN_SHAPES = {(256, 256), (16, 16), (64, 64), (4, 16), (16, 64)}


def window_attention(q, k, v, scale):
    """Hiera's windowed attention on the dedicated kernels (vg_window_attention): q [Bw, wq, H, D], k / v [Bw, wk, H, D] strided
    views (head dim contiguous).  Returns None for shapes those kernels do not take (the caller falls back to vg_attention)."""
    Bw, wq, H, D = q.shape
    wk = k.shape[1]
    ok = (q.dtype == torch.bfloat16 and (wq, wk) in _WIN_SHAPES and k.shape == (Bw, wk, H, D) and v.shape == k.shape
          and all(t.stride(3) == 1 for t in (q, k, v)) and (D == 72 or (wq == 256 and D in (64, 80))) and (wq != 256 or Bw <= 65535))
    if not ok:
        return None
    lib = _lib.load()
    out = torch.empty(Bw, wq, H, D, dtype=q.dtype, device=q.device)
    rc = lib.vg_window_attention(_p(q), _p(k), _p(v), _p(out), Bw, H, wq, wk, D, q.stride(0), q.stride(1), q.stride(2),
                                 k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
                                 out.stride(0), out.stride(1), out.stride(2), float(scale), _dt(q), _stream())
    _lib.check(rc, "vg_window_attention")
    return out


def attention_windows(q, k, v, scale):
    """Self-attention inside many small independent windows: q/k/v [Bw, wtok, H, D] views of one fused projection.
    Windows are packed back to back into 128-token sequences under a block-diagonal mask (vg_attention, causal = -wtok),
    so a 16-token window costs 1/8 of a query tile instead of a whole padded one.  Falls back to attention() when the
    windows do not pack (wtok >= 128, odd strides, or a window count that is not a multiple of the pack)."""
    Bw, wtok, H, D = q.shape
    out = window_attention(q, k, v, scale)
    if out is not None:
        return out
    pack = 128 // wtok if wtok > 0 else 0
    ok = (pack >= 2 and Bw % pack == 0 and k.shape == q.shape and v.shape == q.shape
          and all(t.stride(0) == wtok * t.stride(1) and t.stride(3) == 1 for t in (q, k, v)))
    if not ok:
        return attention(q, k, v, scale)
    lib = _lib.load()
    B, S = Bw // pack, pack * wtok
    out = torch.empty(Bw, wtok, H, D, dtype=q.dtype, device=q.device)
    rc = lib.vg_attention_splitkv(_p(q), _p(k), _p(v), _p(out), B, H, H, S, S, D,
                                  S * q.stride(1), q.stride(1), q.stride(2), S * k.stride(1), k.stride(1), k.stride(2),
                                  S * v.stride(1), v.stride(1), v.stride(2), S * H * D, H * D, D,
                                  float(scale), -wtok, _dt(q), None, 0, 1, None, _stream())
    _lib.check(rc, "vg_attention(windows)")
    return out


def attention_decode(q, k_cache, v_cache, pos_dev, scale, window=0):
    """One decode step against a growing KV cache: q [1,1,Hq,D]; k_cache/v_cache [max_len,Hkv,D]; the number of valid
    keys is *pos_dev + 1, read on the device (graph-replayable).  The split geometry is fixed by max_len."""
    lib = _lib.load()
    _, Sq, Hq, D = q.shape
    max_len, Hkv = k_cache.shape[0], k_cache.shape[1]
    out = torch.empty(1, Sq, Hq, D, dtype=q.dtype, device=q.device)
    nsplit = max(1, min(64, -(-max_len // 64)))   # one 64-key tile per workgroup x Hkv KV heads (GQA-folded rows)
    ws = torch.empty(Hq * nsplit * Sq * (D + 2), dtype=torch.float32, device=q.device)
    rc = lib.vg_attention_splitkv(_p(q), _p(k_cache), _p(v_cache), _p(out), 1, Hq, Hkv, Sq, max_len, D,
                                  q.stride(0), q.stride(1), q.stride(2), 0, k_cache.stride(0), k_cache.stride(1),
                                  0, v_cache.stride(0), v_cache.stride(1), out.stride(0), out.stride(1), out.stride(2),
                                  float(scale), _causal_code(True, window), _dt(q), _p(ws), ws.numel(), nsplit, _p(pos_dev), _stream())
    _lib.check(rc, "vg_attention_splitkv(decode)")
    return out


def rope_kv_append_(qkv, k_cache, v_cache, cos, sin, H, Hkv, D, pos0=0, pos_dev=None):
    """in place on the fused projection qkv [S,(H+2Hkv)*D]: rotate q, rotate k -> k_cache[pos+s], v -> v_cache[pos+s]."""
    lib = _lib.load()
    S = qkv.shape[0]
    assert qkv.stride(1) == 1 and k_cache.is_contiguous() and v_cache.is_contiguous()
    rc = lib.vg_rope_kv_append(_p(qkv), qkv.stride(0), _p(k_cache), _p(v_cache), _p(_f32(cos)), _p(_f32(sin)), S, H, Hkv, D,
                               int(pos0), _p(pos_dev), _dt(qkv), _stream())
    _lib.check(rc, "vg_rope_kv_append")
    return qkv


def _decode_proj(entry, x, w, mid, norm_w, eps, residual, glu, out_dtype, out, x_code=False):
    """the shared body of the single-row decode projections (decode_gemv / _w8 / _w4): y [1,N] chosen or allocated and checked with the residual,
    then entry(x, w, ldw, *mid, y, norm_w, eps, residual, N, K, glu, [dtype code of x,] dtype code of y, stream)"""
    K = x.shape[-1]
    N = w.shape[0] // 2 if glu else w.shape[0]
    y = out if out is not None else torch.empty(1, N, dtype=out_dtype or x.dtype, device=x.device)
    assert y.is_contiguous() and y.numel() == N
    if residual is not None:
        assert residual.is_contiguous() and residual.numel() == N and residual.dtype == y.dtype
    rc = getattr(_lib.load(), entry)(_p(x), _p(w), w.stride(0), *mid, _p(y), _p(None if norm_w is None else _f32(norm_w)), float(eps),
                                     _p(residual), N, K, int(bool(glu)), *((_dt(x),) if x_code else ()), _dt(y), _stream())
    _lib.check(rc, entry)
    return y


def decode_gemv(x, w, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None, p13=None):
    """Decode-step projection of ONE row: y[N] = rmsnorm(x; norm_w, eps) (or x) @ w^T, optional SwiGLU over w = [gate|up]
    rows and optional residual — HF LlamaRMSNorm + nn.Linear (+ LlamaMLP act) in one launch (vg_decode_gemv).
    p13 = decode_pack13(w): the launch streams those 13-bit rows instead of w (vg_decode_gemv_p13) and gives the same bits."""
    K = x.shape[-1]
    assert x.numel() == K and x.is_contiguous() and w.stride(1) == 1 and w.shape[1] == K
    if p13 is not None:
        return decode_gemv_p13(x, w, *p13, norm_w=norm_w, eps=eps, residual=residual, glu=glu, out_dtype=out_dtype, out=out)
    return _decode_proj("vg_decode_gemv", x, w, (), norm_w, eps, residual, glu, out_dtype, out, x_code=True)


P13_RAW_CAP = 256      # a matrix with more than 1 / P13_RAW_CAP of its rows raw is not packed (decode_pack13)


def decode_pack13(w, raw_cap=True):
    """bf16 [N,K] weight (K a multiple of 2048) -> (packed uint8 [N, K/2048 * 3328], fp32 [N] row scales, int32 [nraw] ascending raw rows): the
    lossless 13-bit rows decode_gemv_p13 streams (vg_decode_pack13, include/vg_kernels.h).  None when raw_cap and more than 1/256 of the rows are raw:
    such a matrix stays on decode_gemv.  One-time load work; reads the raw flags back (a sync)."""
    lib = _lib.load()
    N, K = w.shape
    rb = lib.vg_decode_pack13_row_bytes(int(K))
    assert w.dtype == torch.bfloat16 and w.stride(1) == 1 and rb, "decode_pack13: bf16 rows, K a multiple of 2048"
    packed = torch.empty(N, rb, dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    flag = torch.empty(N, dtype=torch.uint8, device=w.device)
    _lib.check(lib.vg_decode_pack13(_p(w), w.stride(0), N, K, _p(packed), _p(scale), _p(flag), _stream()), "vg_decode_pack13")
    raw = flag.nonzero().view(-1).to(torch.int32)
    if raw_cap and raw.numel() * P13_RAW_CAP > N:
        return None
    return packed, scale, raw


def decode_unpack13(packed, scale, raw, w):
    """the bf16 [N,K] matrix that (packed, scale, raw) of decode_pack13(w) stand for: rows listed in raw come from w (vg_decode_unpack13)"""
    lib = _lib.load()
    N, K = w.shape
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.shape == (N, lib.vg_decode_pack13_row_bytes(int(K)))
    assert scale.dtype == torch.float32 and scale.numel() == N and scale.is_contiguous() and raw.dtype == torch.int32 and raw.is_contiguous()
    assert w.dtype == torch.bfloat16 and w.stride(1) == 1
    out = torch.empty(N, K, dtype=torch.bfloat16, device=w.device)
    rc = lib.vg_decode_unpack13(_p(packed), _p(scale), _p(raw if raw.numel() else None), raw.numel(), _p(w), w.stride(0), _p(out), K, N, K, _stream())
    _lib.check(rc, "vg_decode_unpack13")
    return out


def decode_gemv_p13_supported(K):
    """True when decode_gemv_p13 has the row length K (vg_decode_gemv_p13_supported: 4096, 14336)"""
    return bool(_lib.load().vg_decode_gemv_p13_supported(int(K)))


def decode_gemv_p13(x, w, packed, scale, raw, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """decode_gemv(x, w, ...) bit for bit, streaming decode_pack13(w)'s 13-bit rows instead of w (vg_decode_gemv_p13): x bf16 [1,K]; the rows in
    raw are recomputed from w."""
    K = x.shape[-1]
    assert x.dtype == torch.bfloat16 and x.numel() == K and x.is_contiguous() and w.dtype == torch.bfloat16 and w.stride(1) == 1 and w.shape[1] == K
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.shape == (w.shape[0], K // 2048 * 3328)
    assert scale.dtype == torch.float32 and scale.numel() == w.shape[0] and scale.is_contiguous() and raw.dtype == torch.int32 and raw.is_contiguous()
    mid = (_p(packed), _p(scale), _p(raw if raw.numel() else None), raw.numel())
    return _decode_proj("vg_decode_gemv_p13", x, w, mid, norm_w, eps, residual, glu, out_dtype, out)


def quantize_fp8_rows(w):
    """[N,K] weight -> (uint8 [N,K] holding OCP e4m3 codes, fp32 [N] scales): w ~ scale[n] * fp8.  One-time load work (torch)."""
    wf = w.float()
    scale = (wf.abs().amax(dim=1).clamp_min(1e-12) / 448.0).contiguous()
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    return q, scale


def quantize_fp8(x):
    """activations [M,K] (bf16 / fp32, rows contiguous) -> (uint8 [M,K] e4m3 codes, fp32 [M] row scales) on the device kernel."""
    lib = _lib.load()
    x2, M, ldx = _rows2d(x)
    K = x2.shape[1]
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    _lib.check(lib.vg_quantize_fp8_rows(_p(x2), ldx, _p(q), K, _p(sc), M, K, _dt(x2), _stream()), "vg_quantize_fp8_rows")
    return q, sc


def linear_f8(q, qs, w8, ws, bias=None, residual=None, glu=False, out_dtype=torch.bfloat16):
    """fp8 x fp8 GEMM with row scales on both operands (vg_gemm_f8): q uint8 [M,K] + qs [M]; w8 uint8 [N or 2N, K] + ws."""
    lib = _lib.load()
    M, K = q.shape
    N = w8.shape[0] // 2 if glu else w8.shape[0]
    assert q.dtype == torch.uint8 and w8.dtype == torch.uint8 and w8.shape[1] == K and q.is_contiguous() and w8.stride(1) == 1
    y = torch.empty(M, N, dtype=out_dtype, device=q.device)
    r2 = None
    ldr = 0
    if residual is not None:
        r2, mr, ldr = _rows2d(residual)
        assert r2.dtype == out_dtype and mr == M and r2.shape[1] == N
    rc = lib.vg_gemm_f8(_p(q), K, _p(qs), _p(w8), w8.stride(0), _p(ws), _p(y), N, _p(_f32(bias)), _p(r2), ldr,
                        M, N, K, _dt(y), 1 if glu else 0, _stream())
    _lib.check(rc, "vg_gemm_f8")
    return y


def decode_gemv_w8(x, w8, wscale, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """decode_gemv with fp8 (e4m3) weights + per-row scales (vg_decode_gemv_w8): x bf16 [1,K]; w8 uint8 [N or 2N, K]."""
    K = x.shape[-1]
    assert x.dtype == torch.bfloat16 and x.numel() == K and x.is_contiguous() and w8.dtype == torch.uint8 and w8.stride(1) == 1 and w8.shape[1] == K
    assert wscale.dtype == torch.float32 and wscale.numel() == w8.shape[0] and wscale.is_contiguous()
    return _decode_proj("vg_decode_gemv_w8", x, w8, (_p(wscale),), norm_w, eps, residual, glu, out_dtype, out)


MXFP4_K = {3072: 2, 4096: 2, 8192: 4, 14336: 8}      # row lengths of vg_decode_gemv_w4 -> SPL, scale bytes per lane in a packed row's head
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mxfp4_rows(w):
    """[N,K] weight (K a multiple of 32) -> (uint8 [N,K/2] e2m1 codes, uint8 [N,K/32] e8m0 scales) by the OCP Microscaling v1.0 rule: per block
    of 32 consecutive K elements the scale 2^e, e = floor(log2(amax)) - 2 (clamped to [-127, 127]; byte e + 127; an all-zero block: byte 0 and zero
    codes), the elements w / 2^e rounded to nearest (ties to the even code) onto {0, .5, 1, 1.5, 2, 3, 4, 6}, saturating at 6, sign in bit 3.
    Logical layout: element 2j in the low nibble of byte j (torch.float4_e2m1fn_x2's).  One-time load work (torch, any device)."""
    N, K = w.shape
    assert K % 32 == 0, "MXFP4 blocks are 32 consecutive K elements"
    b = w.float().reshape(N, K // 32, 32)
    amax = b.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)                                # amax = m * 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, (ex - 3).clamp(-127, 127), torch.full_like(ex, -127)).to(torch.int32)
    h = -(e // 2)
    a = torch.ldexp(torch.ldexp(b, h[..., None]), (-e - h)[..., None])     # w / 2^e, exact (two steps: 2^127 and 2^-127 stay normal factors)
    m = a.abs()
    # code = the number of midpoints passed; a tie stays below the midpoints whose lower neighbour is the even code (0 | .5, 1 | 1.5, 2 | 3, 4 | 6)
    code = ((m > 0.25).to(torch.uint8) + (m >= 0.75) + (m > 1.25) + (m >= 1.75) + (m > 2.5) + (m >= 3.5) + (m > 5.0)).to(torch.uint8)
    code = code | (torch.signbit(a).to(torch.uint8) << 3)
    code = code.reshape(N, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).contiguous(), (e + 127).to(torch.uint8).contiguous()


def mxfp4_pack(codes, scales):
    """logical (codes [N,K/2], scales [N,K/32]) -> the packed rows vg_decode_gemv_w4 streams (uint8 [N, 64 * SPL + K/2], include/vg_kernels.h): a
    head of 64 * SPL scale bytes — byte lane * SPL + u = the scale of block 64 u + lane, 0 where there is no such block — then the codes."""
    N, K = codes.shape[0], codes.shape[1] * 2
    assert K in MXFP4_K and scales.shape == (N, K // 32) and codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    spl = MXFP4_K[K]
    head = torch.zeros(N, spl * 64, dtype=torch.uint8, device=codes.device)
    head[:, : K // 32] = scales                              # [u][lane] order, zero-padded to spl * 64 blocks
    head = head.view(N, spl, 64).transpose(1, 2).reshape(N, 64 * spl)
    return torch.cat([head, codes], dim=1).contiguous()


def mxfp4_dequant(codes, scales=None, K=None):
    """the float32 [N,K] tensor an MXFP4 weight means: logical (codes, scales), or packed rows (scales None; K from the row length).  torch, any device."""
    if scales is None:
        K = K or next(k for k, s in MXFP4_K.items() if 64 * s + k // 2 == codes.shape[1])
        spl = MXFP4_K[K]
        head = codes[:, : 64 * spl].reshape(-1, 64, spl).transpose(1, 2).reshape(-1, 64 * spl)
        scales, codes = head[:, : K // 32], codes[:, 64 * spl:]
    N, K = codes.shape[0], codes.shape[1] * 2
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(N, K).long()
    grid = torch.tensor(_E2M1, dtype=torch.float32, device=codes.device)
    val = torch.where((nib & 8) != 0, -grid[nib & 7], grid[nib & 7]).reshape(N, K // 32, 32)
    e = scales.to(torch.int32) - 127
    h = e // 2
    return torch.ldexp(torch.ldexp(val, h[..., None]), (e - h)[..., None]).reshape(N, K)


def decode_gemv_w4(x, w4, scales=None, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """decode_gemv with MXFP4 weights (vg_decode_gemv_w4): x bf16 [1,K]; w4 uint8, N or 2N rows: packed rows (mxfp4_pack; scales None) or the
    logical codes [rows, K/2] with scales uint8 [rows, K/32]."""
    K = x.shape[-1]
    assert x.dtype == torch.bfloat16 and x.numel() == K and x.is_contiguous() and w4.dtype == torch.uint8 and w4.stride(1) == 1
    if scales is not None:
        assert scales.dtype == torch.uint8 and scales.shape == (w4.shape[0], K // 32) and scales.is_contiguous() and w4.shape[1] == K // 2
    else:
        assert K not in MXFP4_K or w4.shape[1] == 64 * MXFP4_K[K] + K // 2, "packed MXFP4 rows of another row length"
    return _decode_proj("vg_decode_gemv_w4", x, w4, (_p(scales),), norm_w, eps, residual, glu, out_dtype, out)


def linear_w4a8_supported(N, K):
    """True when the MXFP4 prefill GEMM covers a [N, K] weight (vg_gemm_w4a8_supported: K a packed row length, N a multiple of 8)."""
    return bool(_lib.load().vg_gemm_w4a8_supported(int(N), int(K)))


def linear_w4a8(q, qs, w4_packed, residual=None, glu=False, out_dtype=torch.bfloat16, out=None):
    """e4m3 activations x MXFP4 weights (vg_gemm_w4a8): q uint8 [M,K] + qs [M] from quantize_fp8; w4_packed uint8 [N or 2N, 64 * SPL + K/2], the packed
    rows of mxfp4_pack read in place (any row stride that is a multiple of 16).  glu: rows [gate; up], y = silu(gate) * up.  q may be row-strided;
    out: a [M,N] destination of out_dtype (rows 16-byte aligned) instead of a new tensor."""
    lib = _lib.load()
    M, K = q.shape
    N = w4_packed.shape[0] // 2 if glu else w4_packed.shape[0]
    assert q.dtype == torch.uint8 and w4_packed.dtype == torch.uint8 and q.stride(1) == 1 and w4_packed.stride(1) == 1
    assert qs.dtype == torch.float32 and qs.numel() == M and qs.is_contiguous()
    assert K not in MXFP4_K or w4_packed.shape[1] == 64 * MXFP4_K[K] + K // 2, "packed MXFP4 rows of another row length"
    y = torch.empty(M, N, dtype=out_dtype, device=q.device) if out is None else out
    assert y.shape == (M, N) and y.dtype == out_dtype and y.stride(1) == 1
    r2 = None
    ldr = 0
    if residual is not None:
        r2, mr, ldr = _rows2d(residual)
        assert r2.dtype == out_dtype and mr == M and r2.shape[1] == N
    rc = lib.vg_gemm_w4a8(_p(q), q.stride(0), _p(qs), _p(w4_packed), w4_packed.stride(0), _p(y), y.stride(0), _p(r2), ldr, M, N, K, _dt(y), 1 if glu else 0, _stream())
    _lib.check(rc, "vg_gemm_w4a8")
    return y


def decode_attention_workspace(H, Hkv, D, max_len, device):
    """zero-filled once: the workspace ends with per-KV-head arrival counters that the kernel resets itself."""
    n = _lib.load().vg_decode_attention_ws_floats(H, Hkv, D, max_len)
    if n < 0:
        raise _lib.VGKernelError(f"vg_decode_attention_ws_floats: bad shape H={H} Hkv={Hkv} D={D} max_len={max_len}")
    return torch.zeros(n, dtype=torch.float32, device=device)


def _decode_attention(fn, qkv, k_cache, v_cache, cos, sin, H, Hkv, D, pos_dev, scale, ws, window, keys_per_wg):
    lib = _lib.load()
    assert qkv.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous() and pos_dev.dtype == torch.int32
    max_len = k_cache.shape[0]
    out = torch.empty(1, H * D, dtype=qkv.dtype, device=qkv.device)
    rc = getattr(lib, fn)(_p(qkv), _p(k_cache), _p(v_cache), _p(_f32(cos)), _p(_f32(sin)), _p(out), H, Hkv, D, max_len,
                          int(window), float(scale), _p(pos_dev), _p(ws), ws.numel(), int(keys_per_wg), _dt(qkv), _stream())
    _lib.check(rc, fn)
    return out


def decode_attention(qkv, k_cache, v_cache, cos, sin, H, Hkv, D, pos_dev, scale, ws, window=0, keys_per_wg=0):
    """Fused RoPE + KV append + attention of the one new token (vg_decode_attention): qkv [1,(H+2Hkv)*D] -> [1,H*D].
    keys_per_wg=128: two 64-key blocks per workgroup (long caches: half the partials to merge)."""
    return _decode_attention("vg_decode_attention", qkv, k_cache, v_cache, cos, sin, H, Hkv, D, pos_dev, scale, ws, window, keys_per_wg)


# ---- fp8 K/V cache: OCP e4m3 codes, one byte per element, no scale, the bf16 cache's [max_len, Hkv, D] layout
def kv_quantize_reference(x):
    """The format's definition as one torch statement (what vg_kv_quantize_fp8 and the kv8 kernels' appends reproduce bit for bit) -> uint8."""
    return x.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def kv_quantize_(src, dst):
    """dst (uint8) <- the e4m3 codes of src (bf16), same number of elements (vg_kv_quantize_fp8); returns dst."""
    assert src.dtype == torch.bfloat16 and dst.dtype == torch.uint8 and src.is_contiguous() and dst.is_contiguous()
    assert src.numel() == dst.numel() and src.device == dst.device
    if src.numel():
        _lib.check(_lib.load().vg_kv_quantize_fp8(_p(src), _p(dst), src.numel(), _stream()), "vg_kv_quantize_fp8")
    return dst


def kv_dequantize(q):
    """uint8 e4m3 codes -> bf16, exact (plain torch; tests and tools)."""
    return q.view(torch.float8_e4m3fn).to(torch.bfloat16)


def decode_attention_kv8_supported(H, Hkv, D, dtype):
    return dtype == torch.bfloat16 and bool(_lib.load().vg_decode_attention_kv8_supported(H, Hkv, D, BF16))


def decode_attention_kv8(qkv, k_cache, v_cache, cos, sin, H, Hkv, D, pos_dev, scale, ws, window=0, keys_per_wg=0):
    """decode_attention on uint8 e4m3 caches (vg_decode_attention_kv8): bit-identical to decode_attention on kv_dequantize of them; the appended
    row is the quantised form of the new key / value.  ws: decode_attention_workspace."""
    assert qkv.dtype == torch.bfloat16 and k_cache.dtype == torch.uint8 and v_cache.dtype == torch.uint8
    return _decode_attention("vg_decode_attention_kv8", qkv, k_cache, v_cache, cos, sin, H, Hkv, D, pos_dev, scale, ws, window, keys_per_wg)


def decode_rope_path(H, Hkv, D, K, dtype):
    """True when vg_decode_qkv_rope + vg_decode_attention2 cover this shape (bf16, head_dim 128: Llama-3)."""
    lib = _lib.load()
    dt = F32 if dtype == torch.float32 else BF16
    return bool(lib.vg_decode_qkv_rope_supported(H, Hkv, D, K, dt) and lib.vg_decode_attention2_supported(H, Hkv, D, dt))


def decode_rope_path_kv8(H, Hkv, D, K, dtype):
    """True when vg_decode_qkv_rope_kv8 + vg_decode_attention2_kv8 cover this shape: decode_rope_path's shapes in bf16 (kv_cache = "fp8_rope")."""
    lib = _lib.load()
    return dtype == torch.bfloat16 and bool(lib.vg_decode_qkv_rope_supported(H, Hkv, D, K, BF16) and lib.vg_decode_attention2_kv8_supported(H, Hkv, D, BF16))


def decode_qkv_rope(x, wqkv, norm_w, eps, k_cache, v_cache, rope_cs, pos_dev, H, Hkv, D, out=None):
    """RMSNorm -> q|k|v GEMV -> RoPE -> KV append of ONE row (vg_decode_qkv_rope): -> rotated q [1, H*D]; k_cache / v_cache row *pos_dev written."""
    assert k_cache.dtype == x.dtype
    return _decode_qkv_rope("vg_decode_qkv_rope", x, wqkv, norm_w, eps, k_cache, v_cache, rope_cs, pos_dev, H, Hkv, D, out)


def decode_qkv_rope_kv8(x, wqkv, norm_w, eps, k_cache, v_cache, rope_cs, pos_dev, H, Hkv, D, out=None):
    """decode_qkv_rope with uint8 e4m3 caches (vg_decode_qkv_rope_kv8): the same q; row *pos_dev of the caches = kv_quantize_reference of the bf16
    rows decode_qkv_rope writes, every other byte untouched."""
    assert x.dtype == torch.bfloat16 and k_cache.dtype == torch.uint8 and v_cache.dtype == torch.uint8
    assert k_cache.shape[1:] == (Hkv, D) and v_cache.shape == k_cache.shape
    return _decode_qkv_rope("vg_decode_qkv_rope_kv8", x, wqkv, norm_w, eps, k_cache, v_cache, rope_cs, pos_dev, H, Hkv, D, out)


def _decode_qkv_rope(fn, x, wqkv, norm_w, eps, k_cache, v_cache, rope_cs, pos_dev, H, Hkv, D, out):
    lib = _lib.load()
    K = x.shape[-1]
    assert x.numel() == K and x.is_contiguous() and wqkv.stride(1) == 1 and wqkv.shape == ((H + 2 * Hkv) * D, K)
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and pos_dev.dtype == torch.int32
    assert rope_cs.dtype == torch.float32 and rope_cs.numel() == D and rope_cs.is_contiguous()
    q = out if out is not None else torch.empty(1, H * D, dtype=x.dtype, device=x.device)
    rc = getattr(lib, fn)(_p(x), _p(wqkv), wqkv.stride(0), _p(_f32(norm_w)), float(eps), _p(q), _p(k_cache), _p(v_cache), _p(rope_cs),
                          _p(pos_dev), H, Hkv, D, K, _dt(x), _stream())
    _lib.check(rc, fn)
    return q


def decode_attention2(q, k_cache, v_cache, H, Hkv, D, pos_dev, scale, ws, window=0, keys_per_wg=256):
    """attention of the one new (pre-rotated) query row against caches that already hold its key / value row (vg_decode_attention2)."""
    return _decode_attention2("vg_decode_attention2", q, k_cache, v_cache, H, Hkv, D, pos_dev, scale, ws, window, keys_per_wg)


def decode_attention2_kv8(q, k_cache, v_cache, H, Hkv, D, pos_dev, scale, ws, window=0, keys_per_wg=256):
    """decode_attention2 on uint8 e4m3 caches (vg_decode_attention2_kv8): bit-identical to decode_attention2 on kv_dequantize of them.  The new
    token's row is in the caches already, so it attends to its own key / value quantised.  ws: decode_attention_workspace."""
    assert q.dtype == torch.bfloat16 and k_cache.dtype == torch.uint8 and v_cache.dtype == torch.uint8
    assert k_cache.shape[1:] == (Hkv, D) and v_cache.shape == k_cache.shape
    return _decode_attention2("vg_decode_attention2_kv8", q, k_cache, v_cache, H, Hkv, D, pos_dev, scale, ws, window, keys_per_wg)


def _decode_attention2(fn, q, k_cache, v_cache, H, Hkv, D, pos_dev, scale, ws, window, keys_per_wg):
    lib = _lib.load()
    assert q.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous() and pos_dev.dtype == torch.int32
    out = torch.empty(1, H * D, dtype=q.dtype, device=q.device)
    rc = getattr(lib, fn)(_p(q), _p(k_cache), _p(v_cache), _p(out), H, Hkv, D, k_cache.shape[0], int(window), float(scale), _p(pos_dev),
                          _p(ws), ws.numel(), int(keys_per_wg), _dt(q), _stream())
    _lib.check(rc, fn)
    return out


def decode_advance_(pos_dev, inc, tok_dev=None, step_dev=None, forced=None, hist=None, raw=None, rope=None):
    """device-side bookkeeping of the decode loop (vg_decode_advance).  tok_dev + step_dev: record / force the emitted token and count the step;
    inc: added to *pos_dev; rope = (cos, sin, rope_cs): refresh the cos / sin row of the (new) position."""
    lib = _lib.load()
    assert pos_dev.dtype == torch.int32 and (tok_dev is None) == (step_dev is None)
    assert tok_dev is None or (tok_dev.dtype == torch.int64 and step_dev.dtype == torch.int32)
    cap = 0 if hist is None else hist.numel()
    assert (raw is None or raw.numel() == cap) and all(t is None or t.dtype == torch.int64 for t in (forced, hist, raw))
    cos, sin, rope_cs = rope if rope is not None else (None, None, None)
    hd = 0
    if rope is not None:
        hd = cos.shape[1]
        assert cos.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous() and rope_cs.numel() == 2 * hd and rope_cs.dtype == torch.float32
    rc = lib.vg_decode_advance(_p(tok_dev), _p(pos_dev), _p(step_dev), _p(forced), 0 if forced is None else forced.numel(), _p(hist), _p(raw), cap,
                               _p(cos), _p(sin), _p(rope_cs), hd, int(inc), _stream())
    _lib.check(rc, "vg_decode_advance")


def decode_step_begin(tok_dev, table, pos_dev, rope=None):
    """x = table[*tok_dev] [1, D] and (rope = (cos, sin, rope_cs)) the cos / sin row of *pos_dev: the head of a captured decode step (vg_decode_step_begin)."""
    lib = _lib.load()
    assert tok_dev.dtype == torch.int64 and table.is_contiguous() and pos_dev.dtype == torch.int32
    D = table.shape[1]
    x = torch.empty(1, D, dtype=table.dtype, device=table.device)
    cos, sin, rope_cs = rope if rope is not None else (None, None, None)
    rc = lib.vg_decode_step_begin(_p(tok_dev), _p(table), _p(x), D, _dt(table), _p(pos_dev), _p(cos), _p(sin), _p(rope_cs), 0 if rope is None else cos.shape[1], _stream())
    _lib.check(rc, "vg_decode_step_begin")
    return x


def argmax_partial(x, acc):
    """first stage of argmax over one long row into the zeroed uint64 accumulator `acc` (int64 tensor [1]); decode_step_end decodes it."""
    lib = _lib.load()
    x = x.contiguous()
    assert acc.dtype == torch.int64 and acc.numel() >= 1
    _lib.check(lib.vg_argmax_partial(_p(x), 1, x.numel(), _p(acc), _dt(x), _stream()), "vg_argmax_partial")


def sampling_params(T, k, p, seed, device, out=None):
    """the 24-byte device parameter block vg_sample reads ({float T; float p; int k; int pad; uint64 seed}) as int32 [6]; `out` is rewritten in
    place (one host-to-device copy, outside any capture), so a captured decode step picks the new values up without a re-capture."""
    import struct
    raw = struct.pack("<ffiiQ", float(T), float(p), int(k), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
    host = torch.frombuffer(bytearray(raw), dtype=torch.int32)
    if out is None:
        out = torch.empty(6, dtype=torch.int32, device=device)
    out.copy_(host)
    return out


def sample_workspace(device):
    """the fast sampling route's workspace (vg_sample_workspace_ints() int32, zero-filled; one per stream, reused by every launch)"""
    return torch.zeros(int(_lib.load().vg_sample_workspace_ints()), dtype=torch.int32, device=device)


def sample_fast_route(k, n):
    """whether vg_sample_partial's fast route covers top_k = k on a row of n entries"""
    return 1 <= int(k) <= 64 and int(k) < n and n <= 131072


def sample_partial(x, params_dev, step_dev, acc=None, tok=None, u_override=None, fast_ws=None):
    """HF's Temperature -> TopK -> TopP warpers + the draw on one fp32 logits row (vg_sample_partial): the drawn entry's packed key into acc
    (int64 [1], decode_step_end's hand-off) and / or its index into tok (int64 [1]).  u_override: device float32 [1] replacing the Philox uniform.
    fast_ws (sample_workspace): the multi-workgroup route for 1 <= k <= 64 (same results; other k fall back inside the launch); None: general route."""
    lib = _lib.load()
    x = x.contiguous().view(-1)
    assert x.dtype == torch.float32 and params_dev.dtype == torch.int32 and params_dev.numel() == 6 and step_dev.dtype == torch.int32
    assert acc is not None or tok is not None
    assert all(t is None or t.dtype == torch.int64 for t in (acc, tok)) and (u_override is None or u_override.dtype == torch.float32)
    assert fast_ws is None or (fast_ws.dtype == torch.int32 and fast_ws.numel() >= lib.vg_sample_workspace_ints())
    rc = lib.vg_sample_partial(_p(x), x.numel(), _p(params_dev), _p(step_dev), _p(u_override), _p(acc), _p(tok), _p(fast_ws), _stream())
    _lib.check(rc, "vg_sample_partial")


def sample_workspace_rows(B, device):
    """B fast-route workspaces in one tensor [B, vg_sample_workspace_ints()] (zero-filled): row b of sample_partial_rows works in slice b"""
    return torch.zeros(int(B), int(_lib.load().vg_sample_workspace_ints()), dtype=torch.int32, device=device)


def sample_partial_rows(logits, params, step, acc=None, tok=None, u_override=None, fast_ws=None):
    """sample_partial on every row of logits [B, V] (fp32, rows contiguous) in one launch (vg_sample_partial_rows): row b with its parameter
    block params[b] (int32 [B, 6]), step word step[b] and, when given, uniform u_override[b]; acc / tok int64 [B].  Row b is bit-identical to
    sample_partial on row b alone.  fast_ws (sample_workspace_rows(B)): the multi-workgroup route, a workspace per row; None: the general route."""
    lib = _lib.load()
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]
    B, n = logits.shape
    assert params.dtype == torch.int32 and params.is_contiguous() and params.numel() >= 6 * B and params.shape[-1] == 6
    assert step.dtype == torch.int32 and step.is_contiguous() and step.numel() >= B
    assert acc is not None or tok is not None
    assert all(t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() >= B) for t in (acc, tok))
    assert u_override is None or (u_override.dtype == torch.float32 and u_override.is_contiguous() and u_override.numel() >= B)
    assert fast_ws is None or (fast_ws.dtype == torch.int32 and fast_ws.is_contiguous() and fast_ws.numel() >= B * lib.vg_sample_workspace_ints())
    rc = lib.vg_sample_partial_rows(_p(logits), logits.stride(0), n, B, _p(params), _p(step), _p(u_override), _p(acc), _p(tok), _p(fast_ws), _stream())
    _lib.check(rc, "vg_sample_partial_rows")


def token_scores_workspace(B, device):
    """token_scores_rows' workspace for B rows: [B, vg_token_scores_workspace_ints()] int32, zero-filled once (row b works in slice b)"""
    return torch.zeros(int(B), int(_lib.load().vg_token_scores_workspace_ints()), dtype=torch.int32, device=device)


def token_scores_rows(logits, step, scores, top2, acc=None, tok=None, ws=None):
    """per-token scores of the B rows of logits [B, V] (fp32, rows contiguous, B <= 16) in one launch (vg_token_scores_rows): slot step[b] of
    scores[b] (float32 [B, cap, 2]) receives (log_softmax(row b)[pick], top-2 margin) and the same slot of top2[b] (int64 [B, cap, 2]) the
    indices (top1, top2).  The pick is the index in the packed key acc[b] (argmax_partial's / sample_partial's hand-off, read only) or tok[b]:
    exactly one of them (int64 [B]).  ws: token_scores_workspace(B), needed for V > 2048.  Row b is bit-identical to the launch on row b alone."""
    lib = _lib.load()
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]
    B, n = logits.shape
    assert step.dtype == torch.int32 and step.is_contiguous() and step.numel() >= B
    assert scores.dtype == torch.float32 and top2.dtype == torch.int64 and scores.is_contiguous() and top2.is_contiguous()
    assert scores.shape == top2.shape and scores.numel() % (2 * B) == 0 and scores.shape[-1] == 2
    cap = scores.numel() // (2 * B)
    assert all(t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() >= B) for t in (acc, tok))
    assert ws is None or (ws.dtype == torch.int32 and ws.is_contiguous() and ws.numel() >= B * lib.vg_token_scores_workspace_ints())
    rc = lib.vg_token_scores_rows(_p(logits), logits.stride(0), n, B, _p(acc), _p(tok), _p(step), _p(scores), _p(top2), cap, _p(ws), _stream())
    _lib.check(rc, "vg_token_scores_rows")


def sample_survivors(x, params_dev):
    """the entries the warpers keep for one fp32 logits row (vg_sample_survivors) -> (indices int64, probabilities fp32), ascending index."""
    lib = _lib.load()
    x = x.contiguous().view(-1)
    assert x.dtype == torch.float32 and params_dev.dtype == torch.int32 and params_dev.numel() == 6
    n = x.numel()
    idx = torch.empty(n, dtype=torch.int64, device=x.device)
    prob = torch.empty(n, dtype=torch.float32, device=x.device)
    count = torch.zeros(1, dtype=torch.int32, device=x.device)
    _lib.check(lib.vg_sample_survivors(_p(x), n, _p(params_dev), _p(idx), _p(prob), n, _p(count), _stream()), "vg_sample_survivors")
    m = int(count)
    idx, prob = idx[:m].cpu(), prob[:m].cpu()
    order = torch.argsort(idx)
    return idx[order], prob[order]


def philox(seeds, steps):
    """word 0 of philox4x32_10(key = seeds[i], counter = (steps[i], 0, 0, 0)) (vg_sample_philox): seeds int64 / steps int32 device tensors."""
    lib = _lib.load()
    assert seeds.dtype == torch.int64 and steps.dtype == torch.int32 and seeds.numel() == steps.numel()
    out = torch.empty(seeds.numel(), dtype=torch.int32, device=seeds.device)
    _lib.check(lib.vg_sample_philox(_p(seeds.contiguous()), _p(steps.contiguous()), seeds.numel(), _p(out), _stream()), "vg_sample_philox")
    return out


def decode_step_end(acc, tok_dev, pos_dev, step_dev, row, hid_all, forced=None, hist=None, raw=None):
    """the tail of a captured decode step (vg_decode_step_end): token from the argmax accumulator, final-norm row into hid_all[*pos], bookkeeping, *pos += 1."""
    lib = _lib.load()
    assert row.is_contiguous() and hid_all.is_contiguous() and row.dtype == hid_all.dtype and row.numel() == hid_all.shape[1]
    cap = 0 if hist is None else hist.numel()
    rc = lib.vg_decode_step_end(_p(acc), _p(tok_dev), _p(pos_dev), _p(step_dev), _p(forced), 0 if forced is None else forced.numel(), _p(hist), _p(raw), cap,
                                _p(row), _p(hid_all), row.numel(), _dt(row), _stream())
    _lib.check(rc, "vg_decode_step_end")


# ---- the batched multi-prompt decode step: B <= 16 rows, row b bit-identical to the single-row kernel on that row alone
def decode_rows_supported(H, Hkv, D, hidden, inter, dtype):
    """True when the B-row decode kernels cover a bf16 Llama layer of this shape (vg_decode_rows_supported)."""
    return dtype == torch.bfloat16 and bool(_lib.load().vg_decode_rows_supported(H, Hkv, D, hidden, inter, BF16))


def _decode_proj_rows(entry, x, w, mid, norm_w, eps, residual, glu, out_dtype, out, x_code=False):
    """the shared body of the B-row decode projections (decode_gemv_*rows / decode_gemm_*rows): x bf16 [B,K] with unit-stride rows, y [B,N] chosen
    or allocated and checked with the residual, then entry(x, ldx, w, ldw, *mid, y, ldy, norm_w, eps, residual, ldr, N, K, B, glu, dtype code of
    y (x_code: of x), stream)"""
    B, K = x.shape
    assert x.stride(1) == 1 and x.dtype == torch.bfloat16 and w.stride(1) == 1
    N = w.shape[0] // 2 if glu else w.shape[0]
    y = out if out is not None else torch.empty(B, N, dtype=out_dtype or x.dtype, device=x.device)
    assert y.shape == (B, N) and y.stride(1) == 1
    ldr = 0
    if residual is not None:
        assert residual.shape == (B, N) and residual.stride(1) == 1 and residual.dtype == y.dtype
        ldr = residual.stride(0)
    rc = getattr(_lib.load(), entry)(_p(x), x.stride(0), _p(w), w.stride(0), *mid, _p(y), y.stride(0), _p(None if norm_w is None else _f32(norm_w)),
                                     float(eps), _p(residual), ldr, N, K, B, int(bool(glu)), _dt(x if x_code else y), _stream())
    _lib.check(rc, entry)
    return y


def decode_gemv_rows(x, w, norm_w=None, eps=0.0, residual=None, glu=False, out=None):
    """decode_gemv on each of the B rows of x [B,K] (vg_decode_gemv_rows): one pass over w for all rows -> [B,N]."""
    assert w.shape[1] == x.shape[1]
    return _decode_proj_rows("vg_decode_gemv_rows", x, w, (), norm_w, eps, residual, glu, None, out, x_code=True)


def decode_gemm_rows_supported(N, K):
    """True when the MFMA B-row projection covers a [N, K] weight (vg_decode_gemm_rows_supported: K of 3072 / 4096 / 8192 / 14336, any N)."""
    return bool(_lib.load().vg_decode_gemm_rows_supported(int(N), int(K)))


def decode_gemm_rows(x, w, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """The decode projection of the B <= 16 rows of x [B,K] on the matrix pipe (vg_decode_gemm_rows; the mode decode_gemv = "mfma") -> [B,N] of
    out_dtype (bf16 | fp32).  Row b equals the one-row call on row b bit for bit."""
    assert w.shape[1] == x.shape[1] and w.dtype == torch.bfloat16
    return _decode_proj_rows("vg_decode_gemm_rows", x, w, (), norm_w, eps, residual, glu, out_dtype, out)


def decode_gemm_w8_rows_supported(N, K):
    """True when the MFMA B-row projection on fp8 weights covers a [N, K] weight (vg_decode_gemm_w8_rows_supported)."""
    return bool(_lib.load().vg_decode_gemm_w8_rows_supported(int(N), int(K)))


def decode_gemm_w8_rows(x, w8, wscale, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """decode_gemm_rows on fp8 (e4m3) weights + per-row scales (vg_decode_gemm_w8_rows; the mode decode_gemv = "mfma_q"): x bf16 [B,K], B <= 16;
    w8 uint8 [N or 2N, K] -> [B,N] of out_dtype (bf16 | fp32).  Row b equals the one-row call on row b bit for bit."""
    assert w8.dtype == torch.uint8 and w8.shape[1] == x.shape[1]
    assert wscale.dtype == torch.float32 and wscale.numel() == w8.shape[0] and wscale.is_contiguous()
    return _decode_proj_rows("vg_decode_gemm_w8_rows", x, w8, (_p(wscale),), norm_w, eps, residual, glu, out_dtype, out)


def decode_gemm_w4_rows_supported(N, K):
    """True when the MFMA B-row projection on packed MXFP4 rows covers a [N, K] weight (vg_decode_gemm_w4_rows_supported)."""
    return bool(_lib.load().vg_decode_gemm_w4_rows_supported(int(N), int(K)))


def decode_gemm_w4_rows(x, w4, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """decode_gemm_rows on the packed MXFP4 rows of mxfp4_pack (vg_decode_gemm_w4_rows; the mode decode_gemv = "mfma_q"): x bf16 [B,K], B <= 16
    -> [B,N] of out_dtype (bf16 | fp32).  Row b equals the one-row call on row b bit for bit; a block with scale byte 0 counts as zero."""
    K = x.shape[1]
    assert w4.dtype == torch.uint8
    assert K not in MXFP4_K or w4.shape[1] == 64 * MXFP4_K[K] + K // 2, "packed MXFP4 rows of another row length"
    return _decode_proj_rows("vg_decode_gemm_w4_rows", x, w4, (), norm_w, eps, residual, glu, out_dtype, out)


def decode_gemv_w8_rows_supported(K):
    """True when the B-row fp8 GEMV has the row length K (vg_decode_gemv_w8_rows_supported: 3072, 4096, 8192, 14336)."""
    return bool(_lib.load().vg_decode_gemv_w8_rows_supported(int(K)))


def decode_gemv_w8_rows(x, w8, wscale, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """decode_gemv_w8 on each of the B rows of x [B,K] (vg_decode_gemv_w8_rows): one pass over the fp8 weights for all rows -> [B,N]."""
    assert w8.dtype == torch.uint8 and w8.shape[1] == x.shape[1]
    assert wscale.dtype == torch.float32 and wscale.numel() == w8.shape[0] and wscale.is_contiguous()
    return _decode_proj_rows("vg_decode_gemv_w8_rows", x, w8, (_p(wscale),), norm_w, eps, residual, glu, out_dtype, out)


def decode_gemv_w4_rows_supported(K):
    """True when the B-row MXFP4 GEMV has the row length K (vg_decode_gemv_w4_rows_supported: 3072, 4096, 8192, 14336)."""
    return bool(_lib.load().vg_decode_gemv_w4_rows_supported(int(K)))


def decode_gemv_w4_rows(x, w4, norm_w=None, eps=0.0, residual=None, glu=False, out_dtype=None, out=None):
    """decode_gemv_w4 on each of the B rows of x [B,K] (vg_decode_gemv_w4_rows): one pass over the packed MXFP4 rows (mxfp4_pack) for all rows
    -> [B,N]."""
    K = x.shape[1]
    assert w4.dtype == torch.uint8
    assert K not in MXFP4_K or w4.shape[1] == 64 * MXFP4_K[K] + K // 2, "packed MXFP4 rows of another row length"
    return _decode_proj_rows("vg_decode_gemv_w4_rows", x, w4, (), norm_w, eps, residual, glu, out_dtype, out)


def decode_qkv_rope_rows(x, wqkv, norm_w, eps, k_slots, v_slots, row0, rope_cs, pos_dev, H, Hkv, D, out=None):
    """decode_qkv_rope on each row of x [B,K]: row b at position pos_dev[b] with rope_cs[b], its K / V rows into slot b of k_slots / v_slots
    ([B, rows, Hkv, D], row j of the sequence at j - row0) -> rotated q [B, H*D]."""
    assert k_slots.dtype == x.dtype
    return _decode_qkv_rope_rows("vg_decode_qkv_rope_rows", x, wqkv, norm_w, eps, k_slots, v_slots, row0, rope_cs, pos_dev, H, Hkv, D, out)


def decode_qkv_rope_rows_kv8(x, wqkv, norm_w, eps, k_slots, v_slots, row0, rope_cs, pos_dev, H, Hkv, D, out=None):
    """decode_qkv_rope_rows with uint8 e4m3 slots (vg_decode_qkv_rope_rows_kv8): row b is decode_qkv_rope_kv8 on that row alone."""
    assert x.dtype == torch.bfloat16 and k_slots.dtype == torch.uint8 and v_slots.dtype == torch.uint8
    return _decode_qkv_rope_rows("vg_decode_qkv_rope_rows_kv8", x, wqkv, norm_w, eps, k_slots, v_slots, row0, rope_cs, pos_dev, H, Hkv, D, out)


def _decode_qkv_rope_rows(fn, x, wqkv, norm_w, eps, k_slots, v_slots, row0, rope_cs, pos_dev, H, Hkv, D, out):
    lib = _lib.load()
    B, K = x.shape
    assert x.stride(1) == 1 and wqkv.stride(1) == 1 and wqkv.shape == ((H + 2 * Hkv) * D, K) and pos_dev.dtype == torch.int32 and pos_dev.numel() >= B
    assert k_slots.is_contiguous() and v_slots.is_contiguous() and k_slots.shape[0] >= B and k_slots.shape[2:] == (Hkv, D) and k_slots.shape == v_slots.shape
    assert rope_cs.dtype == torch.float32 and rope_cs.is_contiguous() and rope_cs.shape[-1] == D and rope_cs.shape[0] >= B
    q = out if out is not None else torch.empty(B, H * D, dtype=x.dtype, device=x.device)
    rc = getattr(lib, fn)(_p(x), x.stride(0), _p(wqkv), wqkv.stride(0), _p(_f32(norm_w)), float(eps), _p(q), q.stride(0), _p(k_slots), _p(v_slots),
                          k_slots.stride(0), int(row0), k_slots.shape[1], _p(rope_cs), _p(pos_dev), H, Hkv, D, K, B, _dt(x), _stream())
    _lib.check(rc, fn)
    return q


def decode_attention2_rows_workspace(H, Hkv, D, n_bound, keys_per_wg, B, device):
    n = _lib.load().vg_decode_attention2_rows_ws_floats(H, Hkv, D, int(n_bound), int(keys_per_wg), int(B))
    if n < 0:
        raise _lib.VGKernelError(f"vg_decode_attention2_rows_ws_floats: bad shape H={H} Hkv={Hkv} D={D} n_bound={n_bound} B={B}")
    return torch.zeros(n, dtype=torch.float32, device=device)


def decode_attention2_rows(q, k_cache, v_cache, k_slots, v_slots, row0, H, Hkv, D, pos_dev, n_bound, scale, ws, window=0, keys_per_wg=256):
    """decode_attention2 on each row of q [B, H*D]: keys [0, row0) from the shared caches, [row0, pos_dev[b]] from slot b -> [B, H*D]."""
    return _decode_attention2_rows("vg_decode_attention2_rows", q, k_cache, v_cache, k_slots, v_slots, row0, H, Hkv, D, pos_dev, n_bound, scale, ws,
                                   window, keys_per_wg)


def decode_attention2_rows_kv8(q, k_cache, v_cache, k_slots, v_slots, row0, H, Hkv, D, pos_dev, n_bound, scale, ws, window=0, keys_per_wg=256):
    """decode_attention2_rows with uint8 e4m3 shared caches and slots (vg_decode_attention2_rows_kv8): each row bit-identical to
    decode_attention2_kv8 on it alone.  ws: decode_attention2_rows_workspace."""
    assert q.dtype == torch.bfloat16 and all(t.dtype == torch.uint8 for t in (k_cache, v_cache, k_slots, v_slots))
    assert k_cache.shape[1:] == (Hkv, D) and v_cache.shape == k_cache.shape and k_slots.shape[2:] == (Hkv, D) and v_slots.shape == k_slots.shape
    return _decode_attention2_rows("vg_decode_attention2_rows_kv8", q, k_cache, v_cache, k_slots, v_slots, row0, H, Hkv, D, pos_dev, n_bound, scale, ws,
                                   window, keys_per_wg)


def _decode_attention2_rows(fn, q, k_cache, v_cache, k_slots, v_slots, row0, H, Hkv, D, pos_dev, n_bound, scale, ws, window, keys_per_wg):
    lib = _lib.load()
    B = q.shape[0]
    assert q.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous() and k_slots.is_contiguous() and v_slots.is_contiguous()
    assert pos_dev.dtype == torch.int32 and k_slots.shape[0] >= B
    out = torch.empty(B, H * D, dtype=q.dtype, device=q.device)
    rc = getattr(lib, fn)(_p(q), _p(k_cache), _p(v_cache), k_cache.shape[0], _p(k_slots), _p(v_slots), k_slots.stride(0), int(row0), k_slots.shape[1],
                          _p(out), H, Hkv, D, int(n_bound), int(window), float(scale), _p(pos_dev), _p(ws), ws.numel(), int(keys_per_wg), B, _dt(q),
                          _stream())
    _lib.check(rc, fn)
    return out


def decode_step_rows_supported(H, Hkv, D, hidden, inter, dtype):
    """True when the B-row kernels cover a layer of the decode_attention step (vg_decode_step_rows_supported: bf16 Phi-3-mini width, MHA, head_dim 96)."""
    return dtype == torch.bfloat16 and bool(_lib.load().vg_decode_step_rows_supported(H, Hkv, D, hidden, inter, BF16))


def decode_attention_rows_workspace(H, Hkv, D, n_bound, B, device):
    n = _lib.load().vg_decode_attention_rows_ws_floats(H, Hkv, D, int(n_bound), int(B))
    if n < 0:
        raise _lib.VGKernelError(f"vg_decode_attention_rows_ws_floats: bad shape H={H} Hkv={Hkv} D={D} n_bound={n_bound} B={B}")
    return torch.zeros(n, dtype=torch.float32, device=device)


def decode_attention_rows(qkv, k_cache, v_cache, k_slots, v_slots, row0, cos, sin, H, Hkv, D, pos_dev, n_bound, scale, ws, window=0, kpw_min=2048):
    """decode_attention on each row of qkv [B, (H+2Hkv)*D] (vg_decode_attention_rows): row b RoPE'd at pos_dev[b], its K / V rows appended into slot b
    of k_slots / v_slots ([B, rows, Hkv, D], sequence row j at j - row0), keys [0, row0) from the shared caches; 128 keys per workgroup for the rows
    at pos_dev[b] >= kpw_min -> [B, H*D]."""
    return _decode_attention_rows("vg_decode_attention_rows", qkv, k_cache, v_cache, k_slots, v_slots, row0, cos, sin, H, Hkv, D, pos_dev, n_bound,
                                  scale, ws, window, kpw_min)


def decode_attention_rows_kv8_supported(H, Hkv, D, dtype):
    return dtype == torch.bfloat16 and bool(_lib.load().vg_decode_attention_rows_kv8_supported(H, Hkv, D, BF16))


def decode_attention_rows_kv8(qkv, k_cache, v_cache, k_slots, v_slots, row0, cos, sin, H, Hkv, D, pos_dev, n_bound, scale, ws, window=0, kpw_min=2048):
    """decode_attention_rows with uint8 e4m3 shared caches and slots (vg_decode_attention_rows_kv8): each row bit-identical to decode_attention_kv8
    on it alone.  ws: decode_attention_rows_workspace."""
    assert qkv.dtype == torch.bfloat16 and all(t.dtype == torch.uint8 for t in (k_cache, v_cache, k_slots, v_slots))
    return _decode_attention_rows("vg_decode_attention_rows_kv8", qkv, k_cache, v_cache, k_slots, v_slots, row0, cos, sin, H, Hkv, D, pos_dev,
                                  n_bound, scale, ws, window, kpw_min)


def _decode_attention_rows(fn, qkv, k_cache, v_cache, k_slots, v_slots, row0, cos, sin, H, Hkv, D, pos_dev, n_bound, scale, ws, window, kpw_min):
    lib = _lib.load()
    B = qkv.shape[0]
    assert qkv.stride(1) == 1 and k_cache.is_contiguous() and v_cache.is_contiguous() and k_slots.is_contiguous() and v_slots.is_contiguous()
    assert pos_dev.dtype == torch.int32 and pos_dev.numel() >= B and k_slots.shape[0] >= B and k_slots.shape == v_slots.shape
    assert k_slots.shape[2:] == (Hkv, D) and qkv.shape[1] == (H + 2 * Hkv) * D
    out = torch.empty(B, H * D, dtype=qkv.dtype, device=qkv.device)
    rc = getattr(lib, fn)(_p(qkv), qkv.stride(0), _p(k_cache), _p(v_cache), k_cache.shape[0], _p(k_slots), _p(v_slots), k_slots.stride(0),
                          int(row0), k_slots.shape[1], _p(_f32(cos)), _p(_f32(sin)), _p(out), H, Hkv, D, int(n_bound), int(window),
                          float(scale), _p(pos_dev), int(kpw_min), _p(ws), ws.numel(), B, _dt(qkv), _stream())
    _lib.check(rc, fn)
    return out


def decode_step_begin_rows(tok_dev, table, pos_dev, rope=None):
    """decode_step_begin per row: x[b] = table[tok_dev[b]] -> [B, D]; rope = (cos, sin, rope_cs [B, 2*half]): rope_cs[b] = cos / sin rows of pos_dev[b]."""
    lib = _lib.load()
    B = tok_dev.numel()
    assert tok_dev.dtype == torch.int64 and table.is_contiguous() and pos_dev.dtype == torch.int32 and pos_dev.numel() >= B
    D = table.shape[1]
    x = torch.empty(B, D, dtype=table.dtype, device=table.device)
    cos, sin, rope_cs = rope if rope is not None else (None, None, None)
    if rope is not None:
        assert rope_cs.is_contiguous() and rope_cs.shape[0] >= B and rope_cs.shape[-1] == 2 * cos.shape[1]
    rc = lib.vg_decode_step_begin_rows(_p(tok_dev), _p(table), _p(x), D, _dt(table), _p(pos_dev), _p(cos), _p(sin), _p(rope_cs),
                                       0 if rope is None else cos.shape[1], B, _stream())
    _lib.check(rc, "vg_decode_step_begin_rows")
    return x


def decode_step_end_rows(acc, tok_dev, pos_dev, step_dev, rows, hid, forced=None, hist=None, raw=None, hid_row0=0):
    """decode_step_end per row b: acc / tok / pos / step [b], final-norm row rows[b] into hid[b][pos[b] - hid_row0] (hid [B, n, D]), forced / hist / raw [B, cap]."""
    lib = _lib.load()
    B, D = rows.shape
    assert rows.is_contiguous() and hid.is_contiguous() and hid.dim() == 3 and hid.shape[0] >= B and hid.shape[2] == D and rows.dtype == hid.dtype
    assert all(t.numel() >= B for t in (acc, tok_dev, pos_dev, step_dev))
    cap = 0 if hist is None else hist.shape[1]
    assert all(t is None or (t.is_contiguous() and t.shape[0] >= B) for t in (forced, hist, raw)) and (raw is None or raw.shape[1] == cap)
    rc = lib.vg_decode_step_end_rows(_p(acc), _p(tok_dev), _p(pos_dev), _p(step_dev), _p(forced), 0 if forced is None else forced.shape[1], _p(hist), _p(raw),
                                     cap, _p(rows), _p(hid), hid.stride(0), int(hid_row0), hid.shape[1], D, _dt(rows), B, _stream())
    _lib.check(rc, "vg_decode_step_end_rows")


def argmax_partial_rows(x, acc):
    """argmax_partial of each row of x [B, n] into acc[b] (one launch; vg_argmax_partial)."""
    lib = _lib.load()
    x = x.contiguous()
    assert acc.dtype == torch.int64 and acc.numel() >= x.shape[0]
    _lib.check(lib.vg_argmax_partial(_p(x), x.shape[0], x.shape[1], _p(acc), _dt(x), _stream()), "vg_argmax_partial")


def decode_layer_roles(H, Hkv, D, hidden, inter, dtype):
    """0 / 1 / 3: which roles vg_decode_layer covers for this shape (0: use decode_attention + decode_gemv)."""
    return int(_lib.load().vg_decode_layer_roles(H, Hkv, D, hidden, inter, F32 if dtype == torch.float32 else BF16))


def decode_layer_flags(n_layers, device):
    """[n_layers, vg_decode_layer_flag_ints()] int32 zeros: one flag region per layer; the caller zero-fills ALL of it once per token."""
    return torch.zeros(n_layers, int(_lib.load().vg_decode_layer_flag_ints()), dtype=torch.int32, device=device)


def decode_layer(qkv, k_cache, v_cache, cos, sin, H, Hkv, D, pos_dev, scale, ws, flags, w_o, resid, window=0, mlp=None):
    """vg_decode_layer: attention + o_proj (+ residual) and, with mlp = (norm_w fp32, eps, W gate|up [2I,hidden], W down [hidden,I]), the
    whole MLP as roles of one launch.  flags: one row of decode_layer_flags(), zeroed since its last use.  -> the layer's output row [1, hidden] (mlp) or the post-attention row (mlp=None)."""
    lib = _lib.load()
    assert qkv.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous() and pos_dev.dtype == torch.int32
    assert w_o.stride(1) == 1 and resid.is_contiguous() and flags.dtype == torch.int32 and flags.is_contiguous()
    hidden = w_o.shape[0]
    o = torch.empty(1, H * D, dtype=qkv.dtype, device=qkv.device)
    y_o = torch.empty(1, hidden, dtype=qkv.dtype, device=qkv.device)
    if mlp is None:
        nw, eps, wgu, wd, act, y, inter = None, 0.0, None, None, None, None, 0
    else:
        nw, eps, wgu, wd = mlp
        inter = wd.shape[1]
        assert wgu.shape == (2 * inter, hidden) and wgu.stride(1) == 1 and wd.stride(1) == 1 and nw.dtype == torch.float32
        act = torch.empty(1, inter, dtype=qkv.dtype, device=qkv.device)
        y = torch.empty(1, hidden, dtype=qkv.dtype, device=qkv.device)
    rc = lib.vg_decode_layer(_p(qkv), _p(k_cache), _p(v_cache), _p(_f32(cos)), _p(_f32(sin)), _p(o), H, Hkv, D, k_cache.shape[0],
                             int(window), float(scale), _p(pos_dev), _p(ws), ws.numel(), _p(flags),
                             _p(w_o), w_o.stride(0), _p(resid), _p(y_o),
                             _p(nw), float(eps), _p(wgu), wgu.stride(0) if wgu is not None else 0, _p(act),
                             _p(wd), wd.stride(0) if wd is not None else 0, _p(y),
                             hidden, inter, _dt(qkv), _stream())
    _lib.check(rc, "vg_decode_layer")
    return y_o if mlp is None else y


def store_row_(src, dst, idx_dev, idx_off=0):
    """dst[*idx_dev + idx_off] = src (one row), index read on the device."""
    lib = _lib.load()
    n = src.numel()
    assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype
    _lib.check(lib.vg_store_row(_p(src), _p(dst), n, _p(idx_dev), int(idx_off), _dt(src), _stream()), "vg_store_row")
    return dst


def add_int_(p, v):
    lib = _lib.load()
    assert p.dtype == torch.int32
    _lib.check(lib.vg_add_int(_p(p), int(v), _stream()), "vg_add_int")
    return p


def twoway_image_update(xpe, x, u2, c2, w2t, bo, ln_w, ln_b, eps, pe, nt, TP):
    """Image side of a two-way block's image -> token cross-attention, fused (vg_twoway_image_update; the algebra is in sam2.py: _i2t_fused):
    xpe, x [Nx, P, 256] bf16 (instance n reads slot n % Nx); u2 [N, 8 TP, 256] bf16; c2 [N, 8 TP] fp32; w2t [N, 256, 8 TP] bf16; pe [P, 256]
    -> (x', x' + pe), each [N, P, 256]."""
    lib = _lib.load()
    Nx, P, C = x.shape
    N = u2.shape[0]
    assert N % Nx == 0 and xpe.shape == x.shape
    assert C == 256 and x.dtype == torch.bfloat16 and TP in (8, 16) and nt <= TP, "vg_twoway_image_update: bf16, 256 channels, <= 16 tokens"
    for t_ in (xpe, x, u2, w2t, pe):
        assert t_.is_contiguous() and t_.dtype == torch.bfloat16
    c2 = _f32(c2).contiguous()
    xo = torch.empty(N, P, C, dtype=x.dtype, device=x.device)
    xpo = torch.empty_like(xo)
    rc = lib.vg_twoway_image_update(_p(xpe), _p(x), _p(u2), _p(c2), _p(w2t), _p(_f32(bo)), _p(_f32(ln_w)), _p(_f32(ln_b)), float(eps), _p(pe),
                                    _p(xo), _p(xpo), N, Nx, P, int(nt), int(TP), _dt(x), _stream())
    _lib.check(rc, "vg_twoway_image_update")
    return xo, xpo


def mask_upscale(x, w0, b0, s1, ln_w, ln_b, eps, w1, b1, s0, hyper, es):
    """Mask decoder output upscaling + hypernetwork product, fused (vg_mask_upscale): x [N, es*es, 256], s1 [Bi, (2es)^2, 64], s0 [Bi, (4es)^2, 32]
    (instance n -> image n % Bi), hyper [N, 4, 32] -> masks fp32 [N, 4, 4es, 4es]."""
    lib = _lib.load()
    N, Bi = x.shape[0], s1.shape[0]
    assert x.dtype == torch.bfloat16 and x.shape[1:] == (es * es, 256) and s1.shape[1:] == (4 * es * es, 64) and s0.shape == (Bi, 16 * es * es, 32)
    assert hyper.shape == (N, 4, 32) and w0.shape == (256, 256) and w1.shape == (128, 64) and N % Bi == 0
    for t_ in (x, w0, s1, w1, s0):
        assert t_.is_contiguous() and t_.dtype == torch.bfloat16
    hyper = hyper.to(torch.bfloat16).contiguous()
    out = torch.empty(N, 4, 4 * es, 4 * es, dtype=torch.float32, device=x.device)
    rc = lib.vg_mask_upscale(_p(x), _p(w0), _p(_f32(b0)), _p(s1), _p(_f32(ln_w)), _p(_f32(ln_b)), float(eps), _p(w1), _p(_f32(b1)), _p(s0), _p(hyper),
                             _p(out), N, Bi, int(es), _dt(x), _stream())
    _lib.check(rc, "vg_mask_upscale")
    return out


def layernorm(x, w, b, eps, out_dtype=None):
    lib = _lib.load()
    x2, M, ldx = _rows2d(x)
    C = x2.shape[1]
    out = torch.empty(*x.shape, dtype=out_dtype or x.dtype, device=x.device)
    rc = lib.vg_layernorm(_p(x2), ldx, _p(_f32(w)), _p(_f32(b)), _p(out), C, M, C, float(eps), _dt(x2), _dt(out), _stream())
    _lib.check(rc, "vg_layernorm")
    return out


def rmsnorm(x, w, eps, out_dtype=None):
    lib = _lib.load()
    x2, M, ldx = _rows2d(x)
    C = x2.shape[1]
    out = torch.empty(*x.shape, dtype=out_dtype or x.dtype, device=x.device)
    rc = lib.vg_rmsnorm(_p(x2), ldx, _p(_f32(w)), _p(out), C, M, C, float(eps), _dt(x2), _dt(out), _stream())
    _lib.check(rc, "vg_rmsnorm")
    return out


def axpby(a, b, alpha=1.0, beta=1.0, out_dtype=None):
    """alpha*a + beta*b, b broadcast over the leading dims of a (b.numel() divides a.numel())."""
    lib = _lib.load()
    a = a.contiguous()
    out = torch.empty(a.shape, dtype=out_dtype or a.dtype, device=a.device)
    if b is None:
        rc = lib.vg_axpby(_p(a), None, _p(out), a.numel(), float(alpha), float(beta), 1, _dt(a), F32, _dt(out), _stream())
    else:
        b = b.contiguous()
        assert a.numel() % max(b.numel(), 1) == 0, (a.shape, b.shape)
        rc = lib.vg_axpby(_p(a), _p(b), _p(out), a.numel(), float(alpha), float(beta), b.numel(), _dt(a), _dt(b),
                          _dt(out), _stream())
    _lib.check(rc, "vg_axpby")
    return out


def add(a, b):
    return axpby(a, b, 1.0, 1.0)


def activation(x, act, out_dtype=None):
    lib = _lib.load()
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    _lib.check(lib.vg_activation(_p(x), _p(out), x.numel(), act, _dt(x), _dt(out), _stream()), "vg_activation")
    return out


def swiglu(gu):
    lib = _lib.load()
    gu = gu.contiguous()
    Fh = gu.shape[-1] // 2
    M = gu.numel() // (2 * Fh)
    out = torch.empty(*gu.shape[:-1], Fh, dtype=gu.dtype, device=gu.device)
    _lib.check(lib.vg_swiglu(_p(gu), _p(out), M, Fh, _dt(gu), _stream()), "vg_swiglu")
    return out


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    lib = _lib.load()
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.check(lib.vg_cast(_p(x), _p(out), x.numel(), _dt(x), _dt(out), _stream()), "vg_cast")
    return out


def where_rows(cond, a, b=None, fill=0.0, out=None):
    """out[n,...] = cond[n] > 0 ? a[n,...] : (b broadcast | fill); cond fp32 [rows].  out: optional destination whose rows (one per cond entry,
    each `inner` contiguous elements) may be strided — a [rows, ...] view into a larger buffer."""
    lib = _lib.load()
    a = a.contiguous()
    cond = cond.contiguous().view(-1)
    rows = cond.numel()
    inner = a.numel() // rows
    ld_out = 0
    if out is None:
        out = torch.empty_like(a)
    else:
        assert out.dtype == a.dtype and out.shape[0] == rows and out.numel() == a.numel() and out[0].is_contiguous()
        ld_out = out.stride(0) if rows > 1 else inner
    bp = 1
    if b is not None:
        b = b.contiguous()
        assert b.dtype == a.dtype
        bp = b.numel()
    rc = lib.vg_where_rows(_p(_f32(cond)), _p(a), _p(b), _p(out), rows, inner, bp, float(fill), ld_out, _dt(a), _stream())
    _lib.check(rc, "vg_where_rows")
    return out


def mask_for_mem(x, binarize, scale, bias, out_dtype):
    lib = _lib.load()
    x = x.contiguous()
    assert x.dtype == torch.float32
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    rc = lib.vg_mask_for_mem(_p(x), _p(out), x.numel(), int(bool(binarize)), float(scale), float(bias), _dt(out), _stream())
    _lib.check(rc, "vg_mask_for_mem")
    return out


def threshold(x):
    lib = _lib.load()
    x = x.contiguous()
    assert x.dtype == torch.float32
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(lib.vg_threshold(_p(x), _p(out), x.numel(), _stream()), "vg_threshold")
    return out


def rope_half_(x, cos, sin, pos0):
    """in place; x: [S,H,D] view (head dim contiguous); cos/sin fp32 [max_pos, D/2]."""
    lib = _lib.load()
    S, H, D = x.shape
    assert x.stride(2) == 1
    rc = lib.vg_rope_half(_p(x), x.stride(0), x.stride(1), _p(_f32(cos)), _p(_f32(sin)), S, H, D, int(pos0), _dt(x), _stream())
    _lib.check(rc, "vg_rope_half")
    return x


def rope_axial_(x, cos, sin, n_rope, n_grid):
    """in place; x: [B,N,C] contiguous; cos/sin fp32 [n_grid, C/2]."""
    lib = _lib.load()
    assert x.is_contiguous()
    B, N, C = x.shape
    rc = lib.vg_rope_axial(_p(x), _p(_f32(cos)), _p(_f32(sin)), B, N, C, int(n_rope), int(n_grid), _dt(x), _stream())
    _lib.check(rc, "vg_rope_axial")
    return x


def rope_axial_heads_(x, heads, cos, sin, n_rope, n_grid):
    """in place on the first heads * Ch columns of x [B, N, >= heads*Ch] (row / batch strides free, columns contiguous; bf16): every head of
    Ch = 2 * cos.shape[1] channels rotated with the one table — q | k of a fused q|k|v projection in one launch."""
    lib = _lib.load()
    B, N, _ = x.shape
    Ch = 2 * cos.shape[1]
    assert x.stride(2) == 1 and x.shape[2] >= heads * Ch and x.dtype == torch.bfloat16
    assert 0 <= int(n_rope) <= N and cos.shape[0] >= int(n_grid) > 0, "vg_rope_axial_heads has no row count to check n_rope against: the wrapper does"
    rc = lib.vg_rope_axial_heads(_p(x), x.stride(1), x.stride(0), _p(_f32(cos)), _p(_f32(sin)), B, heads, Ch, int(n_rope), int(n_grid), _dt(x), _stream())
    _lib.check(rc, "vg_rope_axial_heads")
    return x


def embed(ids, table):
    lib = _lib.load()
    ids = ids.contiguous().view(-1)
    assert ids.dtype == torch.int64 and table.is_contiguous()
    D = table.shape[1]
    out = torch.empty(ids.numel(), D, dtype=table.dtype, device=table.device)
    _lib.check(lib.vg_embed(_p(ids), _p(table), _p(out), ids.numel(), D, _dt(table), _stream()), "vg_embed")
    return out


def argmax(x, out=None):
    lib = _lib.load()
    x = x.contiguous()
    n = x.shape[-1]
    rows = x.numel() // n
    if out is None:
        out = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
    assert out.dtype == torch.int64 and out.numel() == rows and out.is_contiguous()
    _lib.check(lib.vg_argmax(_p(x), rows, n, _p(out), _dt(x), _stream()), "vg_argmax")
    return out


def multimask_select(masks, ious, tokens, mode, delta=0.05, thresh=0.98):
    """masks fp32 [N,4,h,w], ious fp32 [N,4], tokens [N,4,C] -> (mask [N,1,h,w] fp32, iou [N], token [N,C], idx [N] int32)."""
    lib = _lib.load()
    masks, ious, tokens = masks.contiguous(), ious.contiguous(), tokens.contiguous()
    assert masks.dtype == torch.float32 and ious.dtype == torch.float32
    N, _, h, w = masks.shape
    C = tokens.shape[-1]
    om = torch.empty(N, 1, h, w, dtype=torch.float32, device=masks.device)
    oi = torch.empty(N, dtype=torch.float32, device=masks.device)
    ot = torch.empty(N, C, dtype=tokens.dtype, device=masks.device)
    ox = torch.empty(N, dtype=torch.int32, device=masks.device)
    rc = lib.vg_multimask_select(_p(masks), _p(ious), _p(tokens), _p(om), _p(oi), _p(ot), _p(ox), N, h * w, C,
                                 float(delta), float(thresh), int(mode), _dt(tokens), _stream())
    _lib.check(rc, "vg_multimask_select")
    return om, oi, ot, ox


def permute5(x, dims, strides):
    """out (contiguous, shape dims[5]) gathered from x's storage at element strides[5]."""
    lib = _lib.load()
    out = torch.empty(*dims, dtype=x.dtype, device=x.device)
    d = (ctypes.c_int64 * 5)(*dims)
    s = (ctypes.c_int64 * 5)(*strides)
    _lib.check(lib.vg_permute5(_p(x), _p(out), d, s, _dt(x), _stream()), "vg_permute5")
    return out


def im2col(x, kh, kw, stride, pad, kpad):
    lib = _lib.load()
    x = x.contiguous()
    B, H, W, C = x.shape
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    out = torch.empty(B * Ho * Wo, kpad, dtype=x.dtype, device=x.device)
    _lib.check(lib.vg_im2col(_p(x), _p(out), B, H, W, C, kh, kw, stride, pad, kpad, _dt(x), _stream()), "vg_im2col")
    return out, Ho, Wo


def dwconv(x, w, bias, k):
    lib = _lib.load()
    x = x.contiguous()
    B, H, W, C = x.shape
    out = torch.empty_like(x)
    _lib.check(lib.vg_dwconv(_p(x), _p(_f32(w)), _p(_f32(bias)), _p(out), B, H, W, C, k, _dt(x), _stream()), "vg_dwconv")
    return out


def conv3s2_ln_gelu(x, w, bias, ln_w, ln_b, eps):
    """Conv2d(k 3, stride 2, pad 1) + LayerNorm2d + GELU in one pass (vg_conv3s2_ln_gelu): x [B,H,W,Cin] channels-last, w [Cout, Kpad] in
    vg_im2col's column order -> [B,(H+1)/2,(W+1)/2,Cout]; None when the channel pair is not one the kernel is built for."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    if (Cin, Cout) not in ((1, 4), (4, 16)) or w.dtype != x.dtype:
        return None
    lib = _lib.load()
    x = x.contiguous()
    out = torch.empty(B, (H + 1) // 2, (W + 1) // 2, Cout, dtype=x.dtype, device=x.device)
    assert w.stride(1) == 1 and w.shape[1] >= 9 * Cin
    rc = lib.vg_conv3s2_ln_gelu(_p(x), _p(w), w.stride(0), _p(_f32(bias)), _p(_f32(ln_w)), _p(_f32(ln_b)), float(eps), _p(out), B, H, W, Cin, Cout,
                                _dt(x), _stream())
    _lib.check(rc, "vg_conv3s2_ln_gelu")
    return out


def pixel_shuffle2(g, bias, B, H, W, C):
    """g: GEMM output [B*H*W, 4*C] (tap-major) -> [B, 2H, 2W, C] (+bias)."""
    lib = _lib.load()
    g = g.contiguous()
    out = torch.empty(B, 2 * H, 2 * W, C, dtype=g.dtype, device=g.device)
    _lib.check(lib.vg_pixel_shuffle2(_p(g), _p(_f32(bias)), _p(out), B, H, W, C, _dt(g), _stream()), "vg_pixel_shuffle2")
    return out


def pool2(x, is_max):
    """x: [B,H,W,C] view whose pixel stride may exceed C (e.g. the q slice of a fused qkv) -> [B,H/2,W/2,C]."""
    lib = _lib.load()
    B, H, W, C = x.shape
    assert x.stride(3) == 1 and x.stride(1) == W * x.stride(2) and x.stride(0) == H * x.stride(1)
    out = torch.empty(B, H // 2, W // 2, C, dtype=x.dtype, device=x.device)
    _lib.check(lib.vg_pool2(_p(x), _p(out), B, H, W, C, x.stride(2), int(bool(is_max)), _dt(x), _stream()), "vg_pool2")
    return out


def window_partition(x, ws):
    lib = _lib.load()
    x = x.contiguous()
    B, H, W, C = x.shape
    nH, nW = -(-H // ws), -(-W // ws)
    out = torch.empty(B * nH * nW, ws * ws, C, dtype=x.dtype, device=x.device)
    _lib.check(lib.vg_window_partition(_p(x), _p(out), B, H, W, C, ws, _dt(x), _stream()), "vg_window_partition")
    return out


def window_unpartition(win, ws, B, H, W):
    lib = _lib.load()
    win = win.contiguous()
    C = win.shape[-1]
    out = torch.empty(B, H, W, C, dtype=win.dtype, device=win.device)
    _lib.check(lib.vg_window_unpartition(_p(win), _p(out), B, H, W, C, ws, _dt(win), _stream()), "vg_window_unpartition")
    return out


def bilinear(x, Ho, Wo):
    """x: fp32 [N,Hi,Wi] -> [N,Ho,Wo], align_corners=False."""
    lib = _lib.load()
    x = x.contiguous()
    assert x.dtype == torch.float32
    N, Hi, Wi = x.shape
    out = torch.empty(N, Ho, Wo, dtype=torch.float32, device=x.device)
    _lib.check(lib.vg_bilinear(_p(x), _p(out), N, Hi, Wi, Ho, Wo, _stream()), "vg_bilinear")
    return out


def bilinear_mask(x, Ho, Wo):
    """threshold(bilinear(x, Ho, Wo)) in one pass: x fp32 [N,Hi,Wi] -> uint8 [N,Ho,Wo] (1 where the interpolated logit > 0)."""
    lib = _lib.load()
    x = x.contiguous()
    assert x.dtype == torch.float32
    N, Hi, Wi = x.shape
    out = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=x.device)
    _lib.check(lib.vg_bilinear_mask(_p(x), _p(out), N, Hi, Wi, Ho, Wo, _stream()), "vg_bilinear_mask")
    return out


def upsample2_add(lateral, top, out=None):
    lib = _lib.load()
    lateral = lateral.contiguous()
    top = top.contiguous()
    B, H, W, C = top.shape
    if out is None:
        out = torch.empty_like(lateral)
    assert out.is_contiguous() and out.shape == lateral.shape and out.dtype == lateral.dtype
    _lib.check(lib.vg_upsample2_add(_p(lateral), _p(top), _p(out), B, H, W, C, _dt(top), _stream()), "vg_upsample2_add")
    return out


# ---------------------------------------------------------------- mask post-processing / evaluation counts (§8f-2, §8f-4)
def _u8(x):
    """bool / uint8 device tensor -> contiguous uint8 view (bool shares its storage)."""
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    assert x.dtype == torch.uint8, f"masks are bool / uint8, got {x.dtype}"
    return x.contiguous()


def connected_components(mask, connectivity=8):
    """mask [..., H, W] bool/uint8 -> (labels, areas) int32 of the same shape (labels: 1 + smallest pixel index)."""
    lib = _lib.load()
    m = _u8(mask)
    H, W = m.shape[-2:]
    N = m.numel() // (H * W)
    labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    counts = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    _lib.check(lib.vg_connected_components(_p(m), _p(labels), _p(counts), N, H, W, int(connectivity), _stream()), "vg_connected_components")
    return labels, counts


def remove_small_blobs(mask, min_size):
    lib = _lib.load()
    m = _u8(mask)
    H, W = m.shape[-2:]
    N = m.numel() // (H * W)
    ws = torch.empty((2,) + tuple(m.shape), dtype=torch.int32, device=m.device)
    out = torch.empty_like(m)
    _lib.check(lib.vg_remove_small_blobs(_p(m), _p(out), _p(ws[0]), _p(ws[1]), N, H, W, int(min_size), _stream()), "vg_remove_small_blobs")
    return out


def fill_holes(scores, max_area):
    lib = _lib.load()
    x = scores.contiguous()
    assert x.dtype == torch.float32
    H, W = x.shape[-2:]
    N = x.numel() // (H * W)
    ws = torch.empty((2,) + tuple(x.shape), dtype=torch.int32, device=x.device)
    out = torch.empty_like(x)
    _lib.check(lib.vg_fill_holes(_p(x), _p(out), _p(ws[0]), _p(ws[1]), N, H, W, int(max_area), _stream()), "vg_fill_holes")
    return out


def mask_pair_counts(a, b, diagonal=False):
    """a [P, ...], b [G, ...] bool/uint8 with equal trailing shapes -> (inter, union) int64 [P, G]
    ([P] of the pairs (i, i) when diagonal)."""
    lib = _lib.load()
    a, b = _u8(a), _u8(b)
    P, G = a.shape[0], b.shape[0]
    L = a.numel() // P
    assert b.numel() // G == L, "masks of a pair must have the same number of pixels"
    shape = (P,) if diagonal else (P, G)
    inter = torch.empty(shape, dtype=torch.int64, device=a.device)
    uni = torch.empty(shape, dtype=torch.int64, device=a.device)
    _lib.check(lib.vg_mask_pair_counts(_p(a), _p(b), _p(inter), _p(uni), P, G, L, int(bool(diagonal)), _stream()), "vg_mask_pair_counts")
    return inter, uni


def boundary_counts(fg, gt, radius):
    """fg, gt [..., H, W] bool/uint8 -> int64 [N, 4] = (n_fg, n_gt, fg_match, gt_match) per image."""
    lib = _lib.load()
    fg, gt = _u8(fg), _u8(gt)
    assert fg.shape == gt.shape
    H, W = fg.shape[-2:]
    N = fg.numel() // (H * W)
    out = torch.empty((N, 4), dtype=torch.int64, device=fg.device)
    _lib.check(lib.vg_boundary_counts(_p(fg), _p(gt), _p(out), N, H, W, int(radius), _stream()), "vg_boundary_counts")
    return out


def mask_boxes(masks, min_size=0, return_mask=False):
    """masks [..., H, W] bool/uint8 -> int32 [..., 5] = (xmin, ymin, xmax, ymax, area) per mask, maxima inclusive,
    (W, H, -1, -1, 0) for an empty mask.  min_size > 0: the table of the mask after remove_small_blobs(min_size), from
    the union-find's own finalize pass; return_mask adds that filtered uint8 mask (the input itself at min_size 0)."""
    lib = _lib.load()
    m = _u8(masks)
    H, W = m.shape[-2:]
    N = m.numel() // (H * W)
    out = torch.empty(tuple(m.shape[:-2]) + (5,), dtype=torch.int32, device=m.device)
    if min_size <= 0:
        _lib.check(lib.vg_mask_boxes(_p(m), _p(out), N, H, W, _stream()), "vg_mask_boxes")
        return (out, m) if return_mask else out
    ws = torch.empty((2,) + tuple(m.shape), dtype=torch.int32, device=m.device)
    kept = torch.empty_like(m) if return_mask else None
    _lib.check(lib.vg_blob_boxes(_p(m), _p(out), _p(kept), _p(ws[0]), _p(ws[1]), N, H, W, int(min_size), _stream()), "vg_blob_boxes")
    return (out, kept) if return_mask else out


def logit_class_counts(logits, target, ignore_index=255):
    """logits [..., H, W] float32 / bf16, target of the same shape (bool, uint8 or an integer dtype with values in 0..255) ->
    int64 [..., 6] = (inter0, inter1, out0, out1, tgt0, tgt1) per mask: the counts of the reference's
    intersectionAndUnionGPU(logits > 0, target, K=2, ignore_index) for every leading index, in one launch
    (vg_logit_class_counts; the contract is stated at its declaration).  The union is out + tgt - inter."""
    lib = _lib.load()
    assert logits.dtype in (torch.float32, torch.bfloat16), f"logits are float32 / bfloat16, got {logits.dtype}"
    assert logits.dim() >= 2 and logits.shape == target.shape, f"logits {tuple(logits.shape)} and target {tuple(target.shape)} differ in shape"
    if target.dtype not in (torch.bool, torch.uint8):
        assert not target.dtype.is_floating_point and not target.dtype.is_complex, f"targets are bool / integer labels, got {target.dtype}"
        assert target.numel() == 0 or bool(((target >= 0) & (target <= 255)).all()), "target labels must lie in 0..255"
        target = target.to(torch.uint8)
    x, t = logits.contiguous(), _u8(target)
    L = x.shape[-2] * x.shape[-1]
    N = x.numel() // L if L else 0
    out = torch.empty(tuple(x.shape[:-2]) + (6,), dtype=torch.int64, device=x.device)
    _lib.check(lib.vg_logit_class_counts(_p(x), _p(t), _p(out), N, L, _dt(x), int(ignore_index), _stream()), "vg_logit_class_counts")
    return out


def mask_rle(masks):
    """masks [..., H, W] bool/uint8 -> (counts int32 [total], offsets int64 [prod(lead) + 1]): COCO's uncompressed run-length
    code of every mask in mask_to_rle_pytorch's form (column-major pixel order, a leading 0 when pixel 0 is foreground); mask n's
    counts are counts[offsets[n] : offsets[n + 1]].  Count, a cumsum, ONE 8-byte read of the total (it sizes the output), emit."""
    lib = _lib.load()
    m = _u8(masks)
    H, W = m.shape[-2:]
    N = m.numel() // (H * W) if H * W else 0
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=m.device)
    if N == 0:
        return torch.empty(0, dtype=torch.int32, device=m.device), offsets
    ws = torch.empty((N, 4, max(lib.vg_mask_rle_units(H, W), 1)), dtype=torch.int32, device=m.device)
    n_runs = torch.empty(N, dtype=torch.int32, device=m.device)
    _lib.check(lib.vg_mask_rle_count(_p(m), _p(ws), _p(n_runs), N, H, W, _stream()), "vg_mask_rle_count")
    torch.cumsum(n_runs, 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[-1])
    if total >= 2 ** 31:
        raise ValueError(f"mask_rle: {total} runs in one call do not fit int32 indexing; encode fewer masks per call")
    counts = torch.empty(total, dtype=torch.int32, device=m.device)
    _lib.check(lib.vg_mask_rle_emit(_p(m), _p(ws), _p(offsets), _p(counts), N, H, W, _stream()), "vg_mask_rle_emit")
    return counts, offsets


def rle_to_mask(counts, offsets, H, W):
    """counts int32 [total], offsets int64 [n + 1] -> (uint8 [n, H, W] of 0 / 1, status int32 [n]).  status[i] = 1 and mask i all zero when
    a count of code i is negative or its counts do not sum to H * W.  The offsets are checked here (one small read): the kernel reads
    counts through them."""
    lib = _lib.load()
    counts, offsets = counts.contiguous(), offsets.contiguous()
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int64 and counts.dim() == 1 and offsets.dim() == 1 and offsets.numel() >= 1
    n = offsets.numel() - 1
    if not bool((offsets[0] == 0) & (offsets[1:] >= offsets[:-1]).all() & (offsets[-1] == counts.numel())):
        raise ValueError("rle_to_mask: offsets must start at 0, not decrease, and end at len(counts)")
    out = torch.empty((n, H, W), dtype=torch.uint8, device=counts.device)
    status = torch.empty(n, dtype=torch.int32, device=counts.device)
    if n == 0:
        return out, status
    ends = torch.empty_like(counts)
    _lib.check(lib.vg_rle_to_mask(_p(counts), _p(offsets), _p(out), _p(status), _p(ends), n, H, W, _stream()), "vg_rle_to_mask")
    return out, status


# ---------------------------------------------------------------- image pre-processing on the device (§8f-1)
def resample_u8(x, out_size, axis, bounds, coeffs):
    """one pass of Pillow's 8-bit resampler over x [N,H,W,C] uint8; bounds [out,2] / coeffs [out,ksize] int32 on device."""
    lib = _lib.load()
    x = x.contiguous()
    assert x.dtype == torch.uint8 and x.dim() == 4
    assert bounds.dtype == torch.int32 and coeffs.dtype == torch.int32 and bounds.shape == (out_size, 2) and coeffs.shape[0] == out_size
    N, H, W, C = x.shape
    shape = (N, H, out_size, C) if axis == 1 else (N, out_size, W, C)
    out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    rc = lib.vg_resample_u8(_p(x), _p(out), N, H, W, C, int(out_size), int(axis), _p(bounds.contiguous()), _p(coeffs.contiguous()),
                            coeffs.shape[1], _stream())
    _lib.check(rc, "vg_resample_u8")
    return out


def resize_cv_linear_u8(x, Ho, Wo, xi=None, xa=None, yi=None, yb=None):
    """OpenCV's 8-bit INTER_LINEAR resize of x [N,H,W,C] uint8 -> [N,Ho,Wo,C]; index / tap tables int32 [Wo,2] / [Ho,2] on the device
    (None for the exact 2x down-scale, which is OpenCV's area fast path)."""
    lib = _lib.load()
    x = x.contiguous()
    assert x.dtype == torch.uint8 and x.dim() == 4
    N, H, W, C = x.shape
    for t, n in ((xi, Wo), (xa, Wo), (yi, Ho), (yb, Ho)):
        assert t is None or (t.dtype == torch.int32 and t.shape == (n, 2) and t.is_contiguous())
    out = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    rc = lib.vg_resize_cv_linear_u8(_p(x), _p(out), N, H, W, C, int(Ho), int(Wo), _p(xi), _p(xa), _p(yi), _p(yb), _stream())
    _lib.check(rc, "vg_resize_cv_linear_u8")
    return out


def normalize_u8(x, mean, std, mode, crop=None, out_dtype=torch.float32):
    """x [N,H,W,3] uint8 -> [N,3,h,w]; crop = (top, left, h, w); mode 0: fp32 (x - mean) / std, 1: fp64 (x / 255 - mean) / std."""
    lib = _lib.load()
    x = x.contiguous()
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3
    N, H, W, _ = x.shape
    top, left, h, w = crop if crop is not None else (0, 0, H, W)
    out = torch.empty((N, 3, h, w), dtype=out_dtype, device=x.device)
    m = (ctypes.c_double * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_double * 3)(*[float(v) for v in std])
    rc = lib.vg_normalize_u8(_p(x), _p(out), N, H, W, int(top), int(left), int(h), int(w), m, sd, int(mode), _dt(out), _stream())
    _lib.check(rc, "vg_normalize_u8")
    return out
