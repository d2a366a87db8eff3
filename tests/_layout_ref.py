"""Plain-torch side of the spatial / layout / mask-decoder tests (CPU only): input designs, float64 references, honest fp32 statements and wrong kernels.

Shared by tests/test_layout_spatial_gpu.py, tests/test_decoder_fused_gpu.py (the kernels) and tests/test_layout_selfcheck.py (the tests' own power).

Part 1, vg_spatial.hip / vg_pointwise.hip / vg_heads_blockdiag: exact cases.  Inputs are small integers (tests/_exact.py: ints), weights small integers
or dyadic fractions, so every fp32 sum is exact in any order and a kernel's output must equal the float64 statement rounded once (torch.equal).  A case
(class Exact) carries the operands, the expected output on a band of the leading output dimension (all of it for small cases; the head and the tail
for the largest ones, where the second grid-stride pass works), and for every compared element the work item that writes it, counted as the launcher
counts (`item`) with its place inside the item (`slot`).  The launchers cap their grid at 4096 workgroups of 256 (CAP items; vg_heads_blockdiag at
2048): a "past one pass" case has between CAP + 1 and about 1.1 M items, not a multiple of 256, so the second pass is ragged.  The wrong kernels
(mutate) are stated on items: the second pass not written, the second pass computing the first pass's items, the last item dropped; and on the
operation: a border tap read from the clamped pixel, the strip tail written past W, the Kpad tail or a window's padding token left unwritten, >= 0 for
> 0, bilinear's x1 not clamped at the last column.

Part 2, vg_twoway_image_update and vg_mask_upscale: float64 chains that round where the kernels round (twoway_v, upscale_chain with dt = float64),
the same chains in fp32 as the CPU statement (dt = float32) with the wrong kernels as keyword `mutant`, the selector design of the two-way update (every
score a multiple of 128, probabilities exactly bf16(1 / count), v = x + (bf16(y) + bo) known exactly; the final LayerNorm is a _rowwise_ref.norm_case)
and, for random data, a two-level check (TwoLevel): a tight bound that almost all elements meet and a wide one for the elements behind a flipped
intermediate bf16 tie, both with their share cap from the CPU fp32 statement against float64 on the same inputs (x 4), never from a kernel.
"""
import math

import torch
import torch.nn.functional as F

import _exact as E
import _rowwise_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CAP = 4096 * 256              # sp_grid / pw_grid: work items of one grid-stride pass
CAP_BD = 2048 * 256           # vg_heads_blockdiag
SENT = E.SENTINEL
GRID_MUTANTS = ("second-pass items not written", "second pass reading the first pass's inputs", "last work item dropped")


def past_one_pass(n, cap=CAP):
    return cap < n <= 1.1 * cap and n % 256 != 0


def ints(shape, vals=E.VALS, seed=0, dtype=F32):
    """E.ints for large shapes too (drawn in pieces of 4 M elements: the int64 indices of a 50 M element case would take 400 MB)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(vals, dtype=dtype)
    n = math.prod(shape)
    out = torch.empty(n, dtype=dtype)
    for i in range(0, n, 1 << 22):
        m = min(n, i + (1 << 22)) - i
        out[i:i + m] = v[torch.randint(len(vals), (m,), generator=g)]
    return out.reshape(tuple(shape))


def once(v64, dtype):
    """float64 -> dtype by ONE rounding; asserts the value was representable in fp32 (the exactness of the design)"""
    y = v64.to(F32)
    assert torch.equal(y.double(), v64), "the design is not exact in fp32"
    return y.to(dtype)


class Exact:
    """name / route; call: the operands the GPU test hands to the entry point; out_shape / out_dtype: the whole output; sel: indices of the leading
    output dimension that `want` covers (None: all); item / slot: per compared element; n_items: as the launcher counts; cap: the grid cap;
    stmt: the CPU fp32 statement's output on the band (tests/_cpu_ops.py where it has one)."""

    def __init__(self, name, route, call, want, item, slot, n_items, sel=None, out_shape=None, cap=CAP, stmt=None, aux=None):
        self.name, self.route, self.call, self.want, self.item, self.slot, self.n_items = name, route, call, want, item, slot, int(n_items)
        self.sel, self.cap, self.stmt, self.aux = sel, cap, stmt, aux or {}
        self.out_shape = tuple(out_shape if out_shape is not None else want.shape)
        self.out_dtype = want.dtype
        assert item.shape == want.shape and slot.shape == want.shape, (name, item.shape, want.shape)
        assert int(item.max()) == self.n_items - 1 or sel is not None, (name, int(item.max()), n_items)

    def band(self, out):
        """the compared part of a whole output"""
        out = out.reshape(self.out_shape)
        return out if self.sel is None else out[self.sel]

    def past(self):
        return self.n_items > self.cap


def _pick(small, bigs, big):
    """the cases of a family: big = True: the small ones and every past-one-pass case; an int: that past-one-pass case alone"""
    if big is True:
        return small + [c for b in bigs for c in b()]
    return bigs[big]()


N_BIG = dict(permute5=2, im2col=1, dwconv=3, shuffle=2, pool2=4, window=2, bilinear=2, conv3s2=2, heads=1)


def _flat(shape, sel=None):
    """flat indices of the (band of the) output, shaped like the band"""
    idx = torch.arange(math.prod(shape)).reshape(shape)
    return idx if sel is None else idx[sel]


def _band(L, sel_big):
    """None for a small leading dimension, else the head and the tail"""
    return None if not sel_big else torch.cat([torch.arange(sel_big[0]), torch.arange(L - sel_big[1], L)])


def equal(case, band, what=""):
    """the assertion of an exact case on the compared band (E.check: explain() as the message)"""
    E.check(band, case.want, what=what or case.name)


def passes(case, band):
    return band.dtype == case.want.dtype and torch.equal(band.reshape(case.want.shape), case.want)


def mutate(case, mutant, honest=None):
    """the band a wrong kernel would leave (honest: the band of an honest kernel, default case.want); None when the mutant does not apply"""
    o = (case.want if honest is None else honest).clone()
    it, sl = case.item, case.slot
    if mutant == GRID_MUTANTS[0]:
        if not case.past():
            return None
        o[it >= case.cap] = SENT
    elif mutant == GRID_MUTANTS[2]:
        o[it == case.n_items - 1] = SENT
    elif mutant == GRID_MUTANTS[1]:
        if not case.past():
            return None
        ns = int(sl.max()) + 1
        key = (it * ns + sl).reshape(-1)
        order = torch.argsort(key)
        ks = key[order]
        second = (it >= case.cap).reshape(-1).nonzero().flatten()
        want_key = key[second] - case.cap * ns
        pos = torch.searchsorted(ks, want_key).clamp(max=ks.numel() - 1)
        found = ks[pos] == want_key
        src = order[pos]
        flat = o.reshape(-1)
        vals = torch.where(found, flat[src], torch.full_like(flat[src], SENT))
        flat[second] = vals
        o = flat.reshape(case.want.shape)
    else:
        f = case.aux.get(mutant)
        if f is None:
            return None
        o = f()
    return o


# ------------------------------------------------------------------ permute5
def permute5_case(name, dims, strides, numel, dtype, seed=0):
    x = ints((numel,), (-3, -2, -1, 1, 2, 3), seed).to(dtype)
    want = torch.as_strided(x, dims, strides).contiguous()
    n = math.prod(dims)
    idx = _flat(dims)
    return Exact(name, "permute5_kernel", dict(x=x, dims=tuple(dims), strides=tuple(strides)), want, idx, torch.zeros_like(idx), n,
                 stmt=torch.as_strided(x, dims, strides).clone(memory_format=torch.contiguous_format))


def permute5_cases(big=True):
    out = []
    for dt in (BF, F32):
        nm = R_NAME[dt]
        B, H, W = 2, 5, 7
        out.append(permute5_case(f"permute5 model gather {nm} B2 5x7", (B, H, W, 3, 1), (3 * H * W, W, 1, H * W, 0), B * 3 * H * W, dt))
        d = (3, 4, 5, 6, 7)          # a true 5-D permutation: the contiguous strides of shape d, permuted by (3, 1, 4, 0, 2)
        st = [math.prod(d[i + 1:]) for i in range(5)]
        p = (3, 1, 4, 0, 2)
        out.append(permute5_case(f"permute5 5-D {nm}", tuple(d[i] for i in p), tuple(st[i] for i in p), math.prod(d), dt, 1))
    if big is not False:
        B, H, W = 2, 420, 420
        bigs = [lambda dt=dt: [permute5_case(f"permute5 model gather {R_NAME[dt]} past one pass", (B, H, W, 3, 1), (3 * H * W, W, 1, H * W, 0), B * 3 * H * W, dt, 2)]
                for dt in (BF, F32)]
        out = _pick(out, bigs, big)
    return out


R_NAME = {BF: "bf16", F32: "fp32"}


# ------------------------------------------------------------------ im2col
def _im2col64(x, kh, kw, stride, pad, kpad, clamp=False, tail=0.0):
    B, H, W, C = x.shape
    xd = x.double().permute(0, 3, 1, 2)
    xp = F.pad(xd, (pad, pad, pad, pad), mode="replicate" if clamp else "constant") if pad else xd
    cols = F.unfold(xp, (kh, kw), stride=stride)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    cols = cols.reshape(B, C, kh * kw, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, kh * kw * C)
    out = torch.full((B * Ho * Wo, kpad), tail, dtype=F64)
    out[:, :kh * kw * C] = cols
    return out


def im2col_case(name, B, H, W, C, k, stride, pad, kpad, dtype, seed=0):
    import _cpu_ops
    x = ints((B, H, W, C), (-3, -2, -1, 1, 2, 3), seed).to(dtype)          # no zero pixel: a wrongly zeroed tap shows
    want = once(_im2col64(x, k, k, stride, pad, kpad), dtype)
    idx = _flat(want.shape)
    aux = {}
    if pad:
        aux["a border tap taken from the clamped pixel instead of skipped"] = lambda: once(_im2col64(x, k, k, stride, pad, kpad, clamp=True), dtype)
    if kpad > k * k * C:
        aux["Kpad tail not zeroed"] = lambda: once(_im2col64(x, k, k, stride, pad, kpad, tail=SENT), dtype)
    return Exact(name, "im2col_kernel", dict(x=x, k=k, stride=stride, pad=pad, kpad=kpad), want, idx, torch.zeros_like(idx), want.numel(),
                 stmt=_cpu_ops.im2col(x, k, k, stride, pad, kpad)[0], aux=aux)


def im2col_cases(big=True):
    out = []
    for dt in (BF, F32):
        nm = R_NAME[dt]
        out.append(im2col_case(f"im2col C3 7x7 s4 p3 Kpad160 {nm} 13x9", 2, 13, 9, 3, 7, 4, 3, 160, dt))
        out.append(im2col_case(f"im2col C3 14x14 s14 p0 {nm} 29x43", 1, 29, 43, 3, 14, 14, 0, 592, dt, 1))
        out.append(im2col_case(f"im2col C16 3x3 s2 p1 Kpad160 {nm} 7x5", 2, 7, 5, 16, 3, 2, 1, 160, dt, 2))
    if big is not False:
        bigs = [lambda: [im2col_case("im2col C3 7x7 s4 p3 Kpad160 bf16 324x324 past one pass", 1, 324, 324, 3, 7, 4, 3, 160, BF, 3)]]
        out = _pick(out, bigs, big)
    return out


# ------------------------------------------------------------------ dwconv
def _dwconv64(x, w, bias, k, clamp=False):
    B, H, W, C = x.shape
    wt = w.double().reshape(k, k, C).permute(2, 0, 1)[:, None]
    xd = x.double().permute(0, 3, 1, 2)
    p = k // 2
    if clamp:          # (replicate padding needs pad < size: pad one pixel at a time)
        for _ in range(p):
            xd = F.pad(xd, (1, 1, 1, 1), mode="replicate")
    else:
        xd = F.pad(xd, (p, p, p, p))
    y = F.conv2d(xd, wt, bias.double() if bias is not None else None, groups=C)
    return y.permute(0, 2, 3, 1).contiguous()


def dwconv_route(dtype, k, C):
    return "dwconv_strip_kernel<7>" if dtype == BF and k == 7 and C % 8 == 0 else "dwconv_kernel"


def dwconv_case(name, B, H, W, C, k, dtype, seed=0, sel_big=None):
    import _cpu_ops
    x = ints((B, H, W, C), (-2, -1, 1, 2), seed).to(dtype)
    w = ints((k * k, C), (-2, -1, 1, 2), seed + 1)
    bias = ints((C,), (-3, -1, 2, 5), seed + 2)
    route = dwconv_route(dtype, k, C)
    sel = _band(B, sel_big)
    xb = x if sel is None else x[sel]
    want = once(_dwconv64(xb, w, bias, k), dtype)
    flat = _flat((B, H, W, C), sel)
    if route == "dwconv_kernel":
        item, slot, n = flat, torch.zeros_like(flat), B * H * W * C
    else:
        c = flat % C
        pix = flat // C
        ox, row = pix % W, pix // W
        WS, CG = (W + 3) // 4, C // 8
        item = (row * WS + ox // 4) * CG + c // 8
        slot = (ox % 4) * 8 + c % 8
        n = B * H * WS * CG
    aux = {"a border tap taken from the clamped pixel instead of skipped": lambda: once(_dwconv64(xb, w, bias, k, clamp=True), dtype)}
    if route != "dwconv_kernel" and W % 4 and sel is None:
        def past_w():          # the strip's pixels ox >= W land on the next row's first pixels (the last row's: past the end)
            Wp = (W + 3) // 4 * 4
            xp = torch.zeros(B, H, Wp, C, dtype=x.dtype)
            xp[:, :, :W] = x
            full = once(_dwconv64(xp, w, bias, k), dtype).reshape(B * H, Wp, C)
            o = want.clone().reshape(B * H * W, C)
            tgt = torch.arange(B * H)[:, None] * W + W + torch.arange(Wp - W)[None, :]
            ok = tgt < B * H * W
            o[tgt[ok]] = full[:, W:][ok]
            return o.reshape(want.shape)
        aux["strip tail pixel written past W"] = past_w
    return Exact(name, route, dict(x=x, w=w, bias=bias, k=k), want, item, slot, n, sel=sel, out_shape=(B, H, W, C),
                 stmt=_cpu_ops.dwconv(xb, w, bias, k), aux=aux)


def dwconv_cases(big=True):
    out = []
    for H in (1, 4, 7):
        for W in (1, 3, 4, 5, 7, 9):
            out.append(dwconv_case(f"dwconv strip bf16 k7 C16 {H}x{W}", 2, H, W, 16, 7, BF, H * 10 + W))
    for k in (3, 5, 7):
        out.append(dwconv_case(f"dwconv scalar fp32 k{k} C5 6x7", 2, 6, 7, 5, k, F32, k))
        out.append(dwconv_case(f"dwconv scalar bf16 k{k} C12 5x9", 2, 5, 9, 12, k, BF, k + 1))
    if big is not False:
        bigs = [lambda: [dwconv_case("dwconv strip bf16 k7 C512 B2731 3x5 past one pass", 2731, 3, 5, 512, 7, BF, 5, sel_big=(2, 3))],
                lambda: [dwconv_case("dwconv scalar bf16 k3 C12 297x295 past one pass", 1, 297, 295, 12, 3, BF, 6)],
                lambda: [dwconv_case("dwconv scalar fp32 k5 C4 513x513 past one pass", 1, 513, 513, 4, 5, F32, 7)]]
        out = _pick(out, bigs, big)
    return out


def dwconv_random(B, H, W, seed=0):
    """random (non-integer) bf16 operands at C = 8 for the strip kernel against the scalar kernel, bit for bit"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, 8, generator=g).to(BF), torch.randn(49, 8, generator=g), torch.randn(8, generator=g))


# ------------------------------------------------------------------ pixel_shuffle2, upsample2_add, pool2
def pixel_shuffle2_case(name, B, H, W, C, dtype, bias=True, seed=0):
    import _cpu_ops
    g = ints((B * H * W, 4 * C), (-3, -2, -1, 1, 2, 3), seed).to(dtype)
    b = ints((C,), (-3, -1, 2, 5), seed + 1) if bias else None
    y = g.double().reshape(B, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, C)
    want = once(y + b.double() if bias else y, dtype)
    idx = _flat(want.shape)
    return Exact(name, "pixel_shuffle2_kernel", dict(g=g, bias=b, B=B, H=H, W=W, C=C), want, idx, torch.zeros_like(idx), want.numel(),
                 stmt=_cpu_ops.pixel_shuffle2(g, b, B, H, W, C))


def upsample2_add_case(name, B, H, W, C, dtype, seed=0):
    import _cpu_ops
    lat = ints((B, 2 * H, 2 * W, C), (-3, -2, -1, 1, 2, 3), seed).to(dtype)
    top = ints((B, H, W, C), (-8, -4, 4, 8), seed + 1).to(dtype)
    want = once(lat.double() + top.double().repeat_interleave(2, 1).repeat_interleave(2, 2), dtype)
    idx = _flat(want.shape)
    return Exact(name, "upsample2_add_kernel", dict(lat=lat, top=top), want, idx, torch.zeros_like(idx), want.numel(), stmt=_cpu_ops.upsample2_add(lat, top))


def shuffle_cases(big=True):
    out = []
    for dt in (BF, F32):
        nm = R_NAME[dt]
        out.append(pixel_shuffle2_case(f"pixel_shuffle2 + bias {nm} 3x5 C6", 2, 3, 5, 6, dt))
        out.append(pixel_shuffle2_case(f"pixel_shuffle2 no bias {nm} 1x1 C3", 1, 1, 1, 3, dt, bias=False, seed=1))
        out.append(upsample2_add_case(f"upsample2_add {nm} 3x5 C6", 2, 3, 5, 6, dt, 2))
    if big is not False:
        bigs = [lambda: [pixel_shuffle2_case("pixel_shuffle2 + bias bf16 181x182 C8 past one pass", 1, 181, 182, 8, BF, seed=3)],
                lambda: [upsample2_add_case("upsample2_add fp32 181x182 C8 past one pass", 1, 181, 182, 8, F32, 4)]]
        out = _pick(out, bigs, big)
    return out


def pool2_case(name, B, H, W, C, Cf, c0, dtype, is_max, seed=0):
    """the [..., c0:c0 + C] view of a fused [B, H, W, Cf] tensor (Cf == C: contiguous)"""
    import _cpu_ops
    vals = (-12, -8, -4, 4, 8, 12) if not is_max else (-3, -2, -1, 1, 2, 3)          # avg: multiples of 4, the mean is an integer
    fused = ints((B, H, W, Cf), vals, seed).to(dtype)
    x = fused[..., c0:c0 + C]
    xd = x.double().permute(0, 3, 1, 2)
    y = (F.max_pool2d(xd, 2, 2) if is_max else F.avg_pool2d(xd, 2, 2)).permute(0, 2, 3, 1).contiguous()
    want = once(y, dtype)
    es = 2 if dtype == BF else 4
    vec = dtype == BF and C % 8 == 0 and Cf % 8 == 0 and (c0 * es) % 16 == 0
    idx = _flat(want.shape)
    k = 8 if vec else 1
    return Exact(name, "pool2_vec8_kernel" if vec else "pool2_kernel", dict(fused=fused, c0=c0, C=C, is_max=is_max), want, idx // k, idx % k,
                 want.numel() // k, stmt=_cpu_ops.pool2(x, is_max))


def pool2_cases(big=True):
    out = []
    for is_max in (True, False):
        m = "max" if is_max else "avg"
        out.append(pool2_case(f"pool2 {m} scalar fp32 C5 contiguous 6x10", 2, 6, 10, 5, 5, 0, F32, is_max))
        out.append(pool2_case(f"pool2 {m} scalar fp32 C5 of 9 strided 6x10", 2, 6, 10, 5, 9, 3, F32, is_max, 1))
        out.append(pool2_case(f"pool2 {m} scalar bf16 C12 contiguous 4x6", 2, 4, 6, 12, 12, 0, BF, is_max, 2))
        out.append(pool2_case(f"pool2 {m} vec8 bf16 C16 contiguous 6x10", 2, 6, 10, 16, 16, 0, BF, is_max, 3))
        out.append(pool2_case(f"pool2 {m} vec8 bf16 C16 of 40 strided 6x10", 2, 6, 10, 16, 40, 8, BF, is_max, 4))
        out.append(pool2_case(f"pool2 {m} bf16 C8 of 24 misaligned view 6x10", 2, 6, 10, 8, 24, 4, BF, is_max, 5))
    if big is not False:
        bigs = [lambda: [pool2_case("pool2 max scalar fp32 C5 of 7 strided 918x914 past one pass", 1, 918, 914, 5, 7, 1, F32, True, 6)],
                lambda: [pool2_case("pool2 avg scalar bf16 C5 contiguous 918x914 past one pass", 1, 918, 914, 5, 5, 0, BF, False, 7)],
                lambda: [pool2_case("pool2 avg vec8 bf16 C16 of 24 strided 1450x1450 past one pass", 1, 1450, 1450, 16, 24, 8, BF, False, 8)],
                lambda: [pool2_case("pool2 max vec8 bf16 C8 contiguous 2054x2046 past one pass", 1, 2054, 2046, 8, 8, 0, BF, True, 9)]]
        out = _pick(out, bigs, big)
    return out


# ------------------------------------------------------------------ windows
def _partition64(x, ws, pad_value=0.0):
    B, H, W, C = x.shape
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    xp = F.pad(x.double(), (0, 0, 0, pw, 0, ph), value=pad_value)
    Hp, Wp = H + ph, W + pw
    return xp.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def window_route(dtype, C):
    return "chunk" if (C * (2 if dtype == BF else 4)) % 16 == 0 else "scalar"


def window_cases_one(name, B, H, W, C, ws, dtype, seed=0):
    """(the partition case, the unpartition case): unpartition of the partition must give the image back"""
    import _cpu_ops
    x = ints((B, H, W, C), (-3, -2, -1, 1, 2, 3), seed).to(dtype)
    win = once(_partition64(x, ws), dtype)
    k = (16 // (2 if dtype == BF else 4)) if window_route(dtype, C) == "chunk" else 1
    idx = _flat(win.shape)
    aux = {}
    if H % ws or W % ws:
        aux["window padding token not zeroed"] = lambda: once(_partition64(x, ws, SENT), dtype)
    part = Exact(name + " partition", "window_part_kernel " + window_route(dtype, C), dict(x=x, ws=ws), win, idx // k, idx % k, win.numel() // k,
                 stmt=_cpu_ops.window_partition(x, ws), aux=aux)
    idx = _flat(x.shape)
    # the padding tokens of the windows handed to unpartition hold garbage: they must not be read into the image
    garbage = once(_partition64(x, ws, 2.0 ** 10), dtype)
    unp = Exact(name + " unpartition", "window_part_kernel reverse " + window_route(dtype, C), dict(win=garbage, ws=ws, B=B, H=H, W=W), x.clone(), idx // k, idx % k,
                x.numel() // k, stmt=_cpu_ops.window_unpartition(garbage, ws, B, H, W))
    return part, unp


def window_cases(big=True):
    out = []
    for ws, H, W in ((4, 6, 9), (7, 10, 15), (8, 13, 17), (8, 16, 8)):
        for dt, C in ((BF, 4), (BF, 12), (F32, 1), (F32, 3), (BF, 8), (F32, 8)):
            out += window_cases_one(f"window ws{ws} {R_NAME[dt]} C{C} {H}x{W}", 2, H, W, C, ws, dt, ws + C)
    if big is not False:
        bigs = [lambda: list(window_cases_one("window ws7 bf16 C12 297x297 past one pass", 1, 297, 297, 12, 7, BF, 30)),
                lambda: list(window_cases_one("window ws8 bf16 C8 1025x1025 past one pass", 1, 1025, 1025, 8, 8, BF, 31))]
        out = _pick(out, bigs, big)
    return out


# ------------------------------------------------------------------ bilinear / bilinear_mask
def bilinear64(x, Ho, Wo, clamp_x1=True):
    """upsample_bilinear2d, align_corners = False, in float64 on x [N, Hi, Wi]; clamp_x1 = False: the wrong kernel that reads the element after the
    row's last one (the next row's first; a zero after the image's last row)"""
    N, Hi, Wi = x.shape
    xd = torch.cat([x.double().reshape(N, -1), torch.zeros(N, 1, dtype=F64)], dim=1)
    fy = ((torch.arange(Ho, dtype=F64) + 0.5) * (Hi / Ho) - 0.5).clamp_min(0.0)
    fx = ((torch.arange(Wo, dtype=F64) + 0.5) * (Wi / Wo) - 0.5).clamp_min(0.0)
    y0, x0 = fy.floor().long(), fx.floor().long()
    y1 = y0 + (y0 < Hi - 1).long()
    x1 = x0 + ((x0 < Wi - 1).long() if clamp_x1 else 1)
    ly, lx = (fy - y0)[:, None], (fx - x0)[None, :]
    g = lambda yy, xx: xd[:, (yy[:, None] * Wi + xx[None, :]).reshape(-1)].reshape(N, Ho, Wo)          # noqa: E731
    return (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))


def bilinear_logits(N, Hi, Wi, seed=0):
    """integer logits with runs of zeros and (a, -3 a) neighbours: at dyadic scales many interpolated values are exactly 0"""
    v = ints((N, Hi, Wi), (-3, -1, 0, 0, 1, 3), seed)
    v[:, :, max(1, Wi // 3 - 1): max(1, Wi // 3 - 1) + max(2, Wi // 8)] = 0.0
    # a row ends in 1 and the next begins with -3: a kernel whose x1 runs past the last column blends them to <= 0 where the clamped value is 1
    v[:, :, -1] = 1.0
    v[:, :, 0] = -3.0
    return v


def bilinear_cases_one(name, N, Hi, Wi, Ho, Wo, seed=0):
    """(the vg_bilinear case, the vg_bilinear_mask case)"""
    import _cpu_ops
    for a, b in ((Hi, Ho), (Wi, Wo)):
        assert b in (2 * a, 4 * a) or a == 2 * b, "a dyadic scale"
    x = bilinear_logits(N, Hi, Wi, seed)
    ref = bilinear64(x, Ho, Wo)
    want = once(ref, F32)
    zeros = float((ref == 0).double().mean())
    assert zeros > 0.02, (name, zeros)          # the strict > 0 is tested on these
    idx = _flat(want.shape)
    up = Wo > Wi
    aux = {"bilinear x1 not clamped at the last column": (lambda: once(bilinear64(x, Ho, Wo, False), F32))} if up else {}
    lin = Exact(name + " bilinear", "bilinear_kernel", dict(x=x, Ho=Ho, Wo=Wo), want, idx, torch.zeros_like(idx), want.numel(), stmt=_cpu_ops.bilinear(x, Ho, Wo),
                aux=aux)
    rows = Wi <= 2048
    Wq = (Wo + 3) // 4
    ox = idx % Wo
    oy, gpr = (idx // Wo) % Ho, (Ho + 3) // 4
    # the rows kernel: a workgroup per group of 4 output rows and no grid cap; the fallback: an item per 4 pixels of a row
    item = (idx // (Ho * Wo)) * gpr + oy // 4 if rows else (idx // Wo) * Wq + ox // 4
    aux = {"`>= 0` for `> 0`": lambda: (ref >= 0).to(torch.uint8)}
    if up:
        aux["bilinear x1 not clamped at the last column"] = lambda: (bilinear64(x, Ho, Wo, False) > 0).to(torch.uint8)
    mask = Exact(name + " bilinear_mask", "bilinear_mask_rows_kernel" if rows else "bilinear_mask_kernel", dict(x=x, Ho=Ho, Wo=Wo), (ref > 0).to(torch.uint8),
                 item, (oy % 4) * Wo + ox if rows else ox % 4, N * gpr if rows else N * Ho * Wq, cap=1 << 40 if rows else CAP,
                 stmt=_cpu_ops.bilinear_mask(x, Ho, Wo), aux=aux)
    return lin, mask


def bilinear_cases(big=True):
    out = []
    out += bilinear_cases_one("x2 5x7 -> 10x14", 2, 5, 7, 10, 14)               # Wo % 4 = 2 (byte stores), Ho % 4 = 2 (a ragged last row group)
    out += bilinear_cases_one("x4 3x5 -> 12x20", 1, 3, 5, 12, 20, 1)
    out += bilinear_cases_one("x1/2 8x12 -> 4x6", 2, 8, 12, 4, 6, 2)
    out += bilinear_cases_one("Wi 2048 on the rows kernel 3x2048 -> 6x4096", 1, 3, 2048, 6, 4096, 4)
    out += bilinear_cases_one("Wi 2052 on the fallback 4x2052 -> 2x1026", 2, 4, 2052, 2, 1026, 5)      # Wo % 4 = 2
    out += bilinear_cases_one("Wi 2052 on the fallback 3x2052 -> 6x4104", 1, 3, 2052, 6, 4104, 6)
    if big is not False:
        bigs = [lambda: list(bilinear_cases_one("fallback 2046x2052 -> 1023x4104 past one pass", 1, 2046, 2052, 1023, 4104, 7)[1:]),
                lambda: list(bilinear_cases_one("511x515 -> 1022x1030 past one pass", 1, 511, 515, 1022, 1030, 8)[:1])]
        out = _pick(out, bigs, big)
    return out


# ------------------------------------------------------------------ conv3s2_ln_gelu
def conv3s2_sums64(x, w, bias, clamp=False):
    """the convolution sums in float64 (exact integers): x [B, H, W, Cin], w [Cout, ldw] with column (ky * 3 + kx) * Cin + c"""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    wt = w.double()[:, :9 * Cin].reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    xd = x.double().permute(0, 3, 1, 2)
    # pad 1 on every side; a stride-2 window that starts at -1 never reaches past H (odd H: the last window ends at H - 1 + 1)
    xd = F.pad(xd, (1, 1, 1, 1), mode="replicate" if clamp else "constant")
    return F.conv2d(xd, wt, bias.double(), stride=2)[:, :, :(H + 1) // 2, :(W + 1) // 2].permute(0, 2, 3, 1).contiguous()


def gelu64(a):
    return a * 0.5 * torch.special.erfc(-a / math.sqrt(2.0))


def conv3s2_case(name, B, H, W, Cin, Cout, dtype, seed=0, sel_big=None):
    """-> (Exact-like operands holder, the _rowwise_ref.Case of LayerNorm + GELU on the exact sums)"""
    x = ints((B, H, W, Cin), (-2, -1, 1, 2), seed).to(dtype)
    w = torch.zeros(Cout, 16 * ((9 * Cin + 15) // 16))          # ldw padded as the model's im2col weights are
    w[:, :9 * Cin] = ints((Cout, 9 * Cin), (-2, -1, 1, 2), seed + 1)
    w = w.to(dtype)
    bias = ints((Cout,), (-3, -1, 2, 5), seed + 2)
    lw, lb = R.norm_weights(Cout, seed)
    eps = 1e-6
    sel = _band(B, sel_big)
    xb = x if sel is None else x[sel]
    case = _conv3s2_rcase(name, conv3s2_sums64(xb, w, bias), lw, lb, eps, dtype)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    flat = _flat((B, Ho, Wo, Cout), sel)
    aux = {"a border tap taken from the clamped pixel instead of skipped": lambda: conv3s2_stmt(conv3s2_sums64(xb, w, bias, clamp=True), lw, lb, eps).to(dtype)}
    ex = Exact(name, f"conv3s2_ln_gelu_kernel<{Cin},{Cout}>", dict(x=x, w=w, bias=bias, lw=lw, lb=lb, eps=eps), case.cpu32.to(dtype).reshape(flat.shape),
               flat // Cout, flat % Cout, B * Ho * Wo, sel=sel, out_shape=(B, Ho, Wo, Cout), stmt=case.cpu32.to(dtype).reshape(flat.shape), aux=aux)
    return ex, case


def conv3s2_stmt(sums64, lw, lb, eps):
    """the CPU fp32 statement (tests/_cpu_ops.py: conv3s2_ln_gelu) on the exact sums"""
    return F.gelu(F.layer_norm(sums64.float(), (sums64.shape[-1],), lw, lb, eps))


def _conv3s2_rcase(name, s, lw, lb, eps, dtype):
    """LayerNorm over the Cout sums, then the erf GELU: unit = 1.13 x the LayerNorm unit (the largest |GELU'|) + the GELU unit, fixed = the GELU's"""
    mean = s.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((s - mean) ** 2).mean(-1, keepdim=True) + eps)
    a = (s - mean) * rstd * lw.double() + lb.double()
    ln_unit = R.U * ((s.abs() + mean.abs()) * rstd * lw.double().abs() + a.abs())
    y = gelu64(a)
    # (the share check counts arguments >= -1, as _rowwise_ref.act_ref does, and not the rows whose variance is 0: there LayerNorm's output is b)
    counted = (a >= -1.0) & (((s - mean) ** 2).sum(-1, keepdim=True) > 0)
    return R.Case(name, [y], [1.13 * ln_unit + R.U * a.abs()], dtype, cpu32=conv3s2_stmt(s, lw, lb, eps), fixed=0.75e-7 * a.abs(), counted=counted,
                  route="conv3s2_ln_gelu")


def conv3s2_cases(big=True):
    out = []
    for dt in (BF, F32):
        for cin, cout in ((1, 4), (4, 16)):
            for H, W in ((1, 1), (7, 9), (2, 2), (12, 31)):
                out.append(conv3s2_case(f"conv3s2 {cin}->{cout} {R_NAME[dt]} {H}x{W}", 3, H, W, cin, cout, dt, H + W))
    if big is not False:
        bigs = [lambda: [conv3s2_case("conv3s2 1->4 bf16 2050x2050 past one pass", 1, 2050, 2050, 1, 4, BF, 9)],
                lambda: [conv3s2_case("conv3s2 4->16 fp32 B4113 30x34 past one pass", 4113, 30, 34, 4, 16, F32, 10, sel_big=(4, 4))]]
        out = _pick(out, bigs, big)
    return out


# ------------------------------------------------------------------ pointwise past the cap
def repeat_tail(n, unit=1, shift=771):
    """index map [n] for 'the part past the first pass repeats the head': elements of the items past CAP copy the elements `shift` items further
    on than where a kernel that re-ran the first pass's items would read (unit: elements per item)"""
    idx = torch.arange(n)
    tail = idx >= CAP * unit
    return torch.where(tail, idx - CAP * unit + shift * unit, idx), tail


def tail_equals_head(out, n, unit=1, shift=771):
    """the check of the repeat_tail design on an output that was prefilled with NaN (a GELU can produce the sentinel 7.0 itself): every element
    written, and the tail bit-equal to the part of the head it repeats"""
    o = out.detach().cpu().reshape(-1)
    src, tail = repeat_tail(n, unit, shift)
    return o.numel() == n and bool(torch.isfinite(o.float()).all()) and torch.equal(o[tail], o[src[tail]])


def tail_mutant(out, n, unit, mutant):
    """what a wrong grid-stride loop leaves of an honest output `out` [n] (items of `unit` elements)"""
    o = out.clone().reshape(-1)
    idx = torch.arange(n)
    if mutant == GRID_MUTANTS[0]:
        o[CAP * unit:] = float("nan")
    elif mutant == GRID_MUTANTS[1]:
        o[CAP * unit:] = o[idx[CAP * unit:] - CAP * unit]
    else:
        o[(n - 1) // unit * unit:] = float("nan")
    return o


def pointwise_n(route_unit, extra=1337):
    """an element count just past one pass of items of `route_unit` elements (not a multiple of 256 items)"""
    n = (CAP + extra) * route_unit
    assert past_one_pass(n // route_unit)
    return n


# ------------------------------------------------------------------ heads_blockdiag
def heads_case(N, nt, TP, dtype, gather, seed=0):
    import _cpu_ops
    if not gather:
        x = ints((N, nt, 128), (-3, -2, -1, 1, 2, 3), seed).to(dtype)
        want = _cpu_ops.heads_blockdiag(x, TP)
        call = dict(x=x, TP=TP)
    else:
        x = ints((N * 8 * TP, 128), (-3, -2, -1, 1, 2, 3), seed).to(dtype)
        want = _cpu_ops.heads_blockdiag_gather(x, N, nt, TP).contiguous()
        call = dict(full=x, N=N, nt=nt, TP=TP)
    idx = _flat(want.shape)
    return Exact(f"heads_blockdiag{' gather' if gather else ''} N{N} nt{nt} TP{TP} {R_NAME[dtype]}", "heads_bd_gather_kernel" if gather else "heads_bd_kernel", call,
                 want, idx, torch.zeros_like(idx), want.numel(), cap=CAP_BD, stmt=want.clone())


def heads_cases(big=True):
    out = []
    for TP in (8, 16):
        for nt in (1, 7, 9, 16):
            if nt <= TP:
                for dt in (BF, F32):
                    out += [heads_case(3, nt, TP, dt, False, nt), heads_case(3, nt, TP, dt, True, nt + 1)]
    if big is not False:
        # (the scatter's count N * 8 * TP * 128 is always a multiple of 256: its second pass cannot be ragged; the gather's is, with N * nt odd)
        bigs = [lambda: list([heads_case(33, 9, 16, BF, False, 20), heads_case(461, 9, 16, BF, True, 21)])]
        out = _pick(out, bigs, big)
    return out


# ====================================================================== part 2: the fused mask-decoder kernels
def _r(v, dt):
    """the bf16 rounding of an intermediate, in the chain's own precision"""
    return R.rbf(v) if dt == F64 else v.to(BF).float()


TWOWAY_MUTANTS = ("two-way: two tokens of one head swapped", "two-way: two heads swapped", "two-way: row r reading row r ^ 1", "two-way: c2 of the neighbouring head",
                  "two-way: token mask at nt - 1", "two-way: n % Nx replaced by n", "two-way: n % Nx replaced by n / (N / Nx)", "two-way: x and xpe exchanged",
                  "two-way: probabilities not rounded to bf16", "two-way: LayerNorm eps x 10", "two-way: one-pass variance")


def twoway_v(d, dt=F64, mutant=None):
    """v = x + (bf16(y) + bo) of vg_twoway_image_update in precision dt (float64: the reference; float32: the CPU statement), the probabilities
    and y rounded to bf16 where the kernel rounds them.  d: dict(xpe, x [Nx, P, 256] bf16, u2 [N, 8 TP, 256] bf16, c2 [N, 8 TP], w2t [N, 256, 8 TP] bf16, bo, nt, TP)."""
    N, Nx, TP, nt = d["u2"].shape[0], d["x"].shape[0], d["TP"], d["nt"]
    P = d["x"].shape[1]
    n = torch.arange(N)
    nx = n % Nx
    if mutant == TWOWAY_MUTANTS[5]:
        nx = n.clamp(max=Nx - 1)          # (the mildest reading: the rows past the last input slot are the last slot's)
    elif mutant == TWOWAY_MUTANTS[6]:
        nx = n // (N // Nx)
    xpe, x = d["xpe"][nx].to(dt), d["x"][nx].to(dt)
    if mutant == TWOWAY_MUTANTS[7]:
        xpe, x = x, xpe
    if mutant == TWOWAY_MUTANTS[2]:
        r = torch.arange(P) ^ 1
        xpe = xpe[:, r.clamp(max=P - 1)]
    u2, c2, w2t = d["u2"].to(dt), d["c2"].to(dt), d["w2t"].to(dt).clone()
    if mutant == TWOWAY_MUTANTS[3]:
        c2 = c2.view(N, 8, TP)[:, [1, 0, 3, 2, 5, 4, 7, 6]].reshape(N, 8 * TP)
    s = (xpe @ u2.transpose(1, 2) + c2[:, None, :]).view(N, P, 8, TP)
    live = nt - 1 if (mutant == TWOWAY_MUTANTS[4] and nt > 1) else nt
    s = s.clone()
    s[..., live:] = float("-inf")
    a = torch.softmax(s, dim=-1)
    if mutant != TWOWAY_MUTANTS[8]:
        a = _r(a, dt)
    if mutant == TWOWAY_MUTANTS[0] and nt > 1:
        a = a.clone()
        a[:, :, 3, [0, nt - 1]] = a[:, :, 3, [nt - 1, 0]]
    if mutant == TWOWAY_MUTANTS[1]:
        a = a[:, :, [0, 1, 2, 3, 4, 6, 5, 7]]
    y = a.reshape(N, P, 8 * TP) @ w2t.transpose(1, 2)
    return x + (_r(y, dt) + d["bo"].to(dt))


def twoway_ln32(v32, lw, lb, eps, mutant=None):
    """the CPU fp32 statement of the final LayerNorm (and its two wrong kernels) -> bf16 x'"""
    if mutant == TWOWAY_MUTANTS[9]:
        eps = eps * 10.0
    if mutant == TWOWAY_MUTANTS[10]:
        mean = v32.mean(-1, keepdim=True)
        var = (v32 * v32).mean(-1, keepdim=True) - mean * mean
        return ((v32 - mean) * torch.rsqrt(var + eps) * lw + lb).to(BF)
    return F.layer_norm(v32, (256,), lw, lb, eps).to(BF)


def twoway_model(d, mutant=None):
    """(x', x' + pe) of the CPU fp32 statement / of a wrong kernel"""
    xo = twoway_ln32(twoway_v(d, F32, mutant), d["lw"], d["lb"], d["eps"], mutant)
    return xo, (xo.float() + d["pe"].float()).to(BF)


def twoway_selector(N, Nx, P, nt, TP, seed=0):
    """the selector design (module docstring).  xpe rows two-hot; u2, c2 in {0, -128}; integer w2t, bo, x; every 8th row of x a `step` row
    (1024 + 8 k: a one-pass variance shows); eps = 0.5 (eps x 10 shows whatever the row); masked columns hold large garbage."""
    g = torch.Generator().manual_seed(seed)
    NC = 8 * TP
    rows = torch.arange(Nx * P)
    ca = (rows * 7 + seed) % 256
    cb = (ca + 1 + (rows * 13) % 255) % 256
    xpe = torch.zeros(Nx * P, 256)
    xpe[rows, ca] = 1.0
    xpe[rows, cb] = 1.0
    xpe = xpe.view(Nx, P, 256)
    u2 = -128.0 * torch.randint(0, 2, (N, 8, TP, 256), generator=g).float()
    c2 = -128.0 * torch.randint(0, 2, (N, 8, TP), generator=g).float()
    w2t = torch.randint(-3, 4, (N, 256, 8, TP), generator=g).float()
    u2[:, :, nt:] = 1000.0          # the masked columns: garbage that must not count
    w2t[..., nt:] = 1000.0
    x = torch.randint(-4, 5, (Nx, P, 256), generator=g).float()
    probes = {}
    x[:, 3::8] = 1024.0 + 8.0 * torch.randint(-2, 3, (Nx, (P - 3 + 7) // 8, 256), generator=g).float()
    bo = torch.randint(-2, 3, (256,), generator=g).float()
    lw, lb = R.norm_weights(256, seed)
    pe = torch.randn(P, 256, generator=g).to(BF)
    d = dict(xpe=xpe.to(BF), x=x.to(BF), u2=u2.view(N, NC, 256).to(BF), c2=c2.view(N, NC), w2t=w2t.view(N, 256, NC).to(BF), bo=bo, lw=lw, lb=lb, eps=0.5, pe=pe,
             nt=nt, TP=TP, N=N, Nx=Nx, P=P)
    for n in range(N):
        for r in range(3, P, 8):
            probes[n * P + r] = "step"
    d["probes"] = probes
    return d


def twoway_selector_case(d, name=""):
    """the exact v (asserted: the fp32 chain reproduces the float64 model with zero error, live probabilities are bf16(1 / count) with count <= TP)
    and the norm_case of the final LayerNorm on it"""
    v64 = twoway_v(d, F64)
    v32 = twoway_v(d, F32)
    assert torch.equal(v32.double(), v64), "the selector design is not exact"
    return R.norm_case(name or "two-way selector", v32.reshape(-1, 256), d["lw"], d["lb"], d["eps"], False, BF, route=f"twoway<{d['TP']}>", probes=d["probes"])


def twoway_random(N, Nx, P, nt, TP, seed=0):
    """random data as test_kernels_gpu.test_twoway_image_update draws it"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale          # noqa: E731
    NC = 8 * TP
    x, pe = rn(Nx, P, 256).to(BF), rn(P, 256).to(BF)
    return dict(xpe=(x.float() + pe.float()).to(BF), x=x, u2=rn(N, NC, 256, scale=0.05).to(BF), c2=rn(N, NC), w2t=rn(N, 256, NC, scale=0.5).to(BF), bo=rn(256),
                lw=1.0 + 0.1 * rn(256), lb=rn(256), eps=1e-5, pe=pe, nt=nt, TP=TP, N=N, Nx=Nx, P=P)


class TwoLevel:
    """ref64; tight [like ref64]: the bound almost every element meets; the CPU statement's output cpu (in the output dtype).  wide = 4 x the
    statement's largest error (floors: 4 x the largest tight bound, 4 x `floor` = the size of one flipped tie from the formats); cap: the share of elements allowed beyond `tight`, a constant of the test — the
    statement's own share must stay under a quarter of it (precondition: a condition on the inputs, asserted before a kernel is looked at)."""

    def __init__(self, name, ref64, tight, cpu, cap, floor=0.0):
        self.name, self.ref, self.tight, self.cap = name, ref64, tight, cap
        e = (cpu.double().reshape(ref64.shape) - ref64).abs()
        self.cpu_max, self.cpu_share = float(e.max()), float((e > tight).double().mean())
        self.wide = 4.0 * max(self.cpu_max, float(tight.max()), floor)

    def precondition(self):
        assert self.cpu_share <= self.cap / 4, f"{self.name}: the fp32 statement's own share {self.cpu_share:.2e} > {self.cap / 4:.2e}: not a case for this cap"

    def evaluate(self, got):
        e = (got.detach().cpu().double().reshape(self.ref.shape) - self.ref).abs()
        worst = float(e.max()) if bool(torch.isfinite(e).all()) else float("inf")
        share = float((~(e <= self.tight)).double().mean())
        return dict(ok=worst <= self.wide and share <= self.cap, worst=worst, wide=self.wide, share=share, cap=self.cap, cpu_max=self.cpu_max, cpu_share=self.cpu_share)

    def check(self, got):
        self.precondition()
        r = self.evaluate(got)
        print(f"TWO {self.name:60s} worst {r['worst']:.3e} of {r['wide']:.3e} (cpu {r['cpu_max']:.3e}) share {r['share']:.2e} cap {r['cap']:.1e} (cpu {r['cpu_share']:.2e})")
        assert r["ok"], (self.name, r)
        return r


TWOWAY_CAP = 2e-3          # twice the share floor of _rowwise_ref: two intermediate bf16 roundings (the probabilities, y) lie under every element; the statement must stay under a quarter
LN_MULT = 16.0          # the slack multiple of the tight LayerNorm bound: the 256-column LayerNorm statements of _rowwise_ref need <= 3.7 units on the CPU, x 4, rounded up


def twoway_random_check(d, name=""):
    """x' of random data against the float64 chain.  tight: 1/2 ulp_bf16 + LN_MULT x the LayerNorm unit of _rowwise_ref on the float64 v; an element
    behind a flipped bf16 tie of a probability or of y lies beyond it (a whole ulp of y moved v) and is counted by the share."""
    v = twoway_v(d, F64).reshape(-1, 256)
    mean = v.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((v - mean) ** 2).mean(-1, keepdim=True) + d["eps"])
    y = (v - mean) * rstd * d["lw"].double() + d["lb"].double()
    slack = LN_MULT * R.U * ((v.abs() + mean.abs()) * rstd * d["lw"].double().abs() + y.abs())
    tight = 0.5 * R.quantum(y.abs() + slack, BF) + slack
    # (the floor of the wide bound: one bf16 ulp of the largest output, about what one flipped tie of y moves an output by)
    return TwoLevel(name or "two-way random", y, tight, twoway_model(d)[0].reshape(-1, 256), TWOWAY_CAP, float(R.quantum(y.abs().max(), BF)))


# ------------------------------------------------------------------ mask upscale
UPSCALE_MUTANTS = ("upscale: tap order (dy, dx) transposed at the first level", "upscale: tap order (dy, dx) transposed at the second level",
                   "upscale: image index n / (N / Bi) for n % Bi", "upscale: LayerNorm over 63 channels", "upscale: eps x 10", "upscale: tanh GELU",
                   "upscale: a missing bf16 rounding")


def _shuffle(g, N, H, W, C, transposed=False):
    """[N, H W, 4 C] (tap-major, tap = dy * 2 + dx) -> [N, 2H * 2W, C]"""
    t = g.reshape(N, H, W, 2, 2, C)
    if transposed:
        t = t.transpose(3, 4)
    return t.permute(0, 1, 3, 2, 4, 5).reshape(N, 4 * H * W, C)


def upscale_chain(d, dt=F64, mutant=None, inst=None, args=None):
    """vg_mask_upscale in precision dt with the kernel's two bf16 roundings (after each GELU) and an fp32 / float64 result [N, 4, 4 es, 4 es]"""
    es, Nall, Bi = d["es"], d["x"].shape[0], d["s1"].shape[0]
    inst = torch.arange(Nall) if inst is None else torch.as_tensor(inst)          # the instances computed (each is independent of the others)
    x, N = d["x"][inst].to(dt), inst.numel()
    img = inst % Bi
    if mutant == UPSCALE_MUTANTS[2]:
        img = inst // (Nall // Bi)
    gelu = gelu64 if dt == F64 else F.gelu
    if mutant == UPSCALE_MUTANTS[5]:
        gelu = lambda t: F.gelu(t, approximate="tanh")          # noqa: E731
    rnd = (lambda t: t) if mutant == UPSCALE_MUTANTS[6] else (lambda t: _r(t, dt))
    g = x @ d["w0"].to(dt).t()
    up = _shuffle(g, N, es, es, 64, mutant == UPSCALE_MUTANTS[0]) + d["b0"].to(dt) + d["s1"].to(dt)[img]
    eps = d["eps"] * (10.0 if mutant == UPSCALE_MUTANTS[4] else 1.0)
    if mutant == UPSCALE_MUTANTS[3]:
        m = up[..., :63].mean(-1, keepdim=True)
        var = ((up[..., :63] - m) ** 2).mean(-1, keepdim=True)
    else:
        m = up.mean(-1, keepdim=True)
        var = ((up - m) ** 2).mean(-1, keepdim=True)
    a = (up - m) * torch.rsqrt(var + eps) * d["lw"].to(dt) + d["lb"].to(dt)
    u = rnd(gelu(a))
    if args is not None:
        args.append(a)
    g = u @ d["w1"].to(dt).t()
    up = _shuffle(g, N, 2 * es, 2 * es, 32, mutant == UPSCALE_MUTANTS[1]) + d["b1"].to(dt) + d["s0"].to(dt)[img]
    if args is not None:
        args.append(up)
    u = _r(gelu(up), dt)
    return (d["hyper"][inst].to(dt) @ u.transpose(1, 2)).view(N, 4, 4 * es, 4 * es)


def upscale_arguments(d):
    """the arguments of the two GELUs in float64"""
    args = []
    upscale_chain(d, F64, args=args)
    return args


def upscale_random(N, Bi, es, seed=0, design="random"):
    """design: 'random' (test_kernels_gpu.test_mask_upscale's draw), 'quiet' (the LayerNorm2d / GELU definition case: rows of small variance, sigma
    about 2^-6, LayerNorm weights that spread the arguments over [-3, 3]), 'saturating' (the index-pinning case: integer operands, every GELU
    argument beyond +-8)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale          # noqa: E731
    P = es * es
    if design == "saturating":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()          # noqa: E731
        x = torch.zeros(N, P, 256)
        pick = torch.randint(0, 256, (N, P, 2), generator=g)
        x.scatter_(2, pick, 1.0)          # one or two ones per pixel: g0 = a sum of one or two integer weight columns
        w0 = ri(-2, 2, 256, 256)
        s1 = ri(-2, 2, Bi, 4 * P, 64)
        # a normalised value is at most sqrt(63) < 7.94: with weight 2 and the offset +-24 alternating by channel every argument lies beyond +-8.1
        lw = torch.full((64,), 2.0)
        lb = torch.where(torch.arange(64) % 2 == 0, 24.0, -24.0)
        # every output of the second product adds / subtracts two live (even) channels: |sum| < 2 x 40, and b1 = +-96 decides the sign
        w1 = torch.zeros(128, 64)
        o = torch.arange(128)
        for j in range(2):
            w1[o, 2 * torch.randint(0, 32, (128,), generator=g)] = ri(0, 1, 128) * 2.0 - 1.0
        b1 = torch.where(torch.arange(32) % 2 == 0, 96.0, -96.0)
        s0 = ri(-2, 2, Bi, 16 * P, 32)
        hyper = ri(-1, 1, N, 4, 32)
        return dict(x=x.to(BF), w0=w0.to(BF), b0=ri(-1, 1, 64), s1=s1.to(BF), lw=lw, lb=lb, eps=1e-6, w1=w1.to(BF), b1=b1, s0=s0.to(BF), hyper=hyper.to(BF), es=es)
    x = rn(N, P, 256).to(BF)
    w0, b0 = rn(256, 256, scale=0.06).to(BF), rn(64, scale=0.1)
    w1, b1 = rn(128, 64, scale=0.12).to(BF), rn(32, scale=0.1)
    s1, s0 = rn(Bi, 4 * P, 64).to(BF), rn(Bi, 16 * P, 32).to(BF)
    lw, lb = 1.0 + 0.1 * rn(64), 0.1 * rn(64)
    if design == "quiet":
        # (no offset, unlike _rowwise_ref's quiet row: 3 + noise cancels in x - mean, and the fp32 statement itself then flips bf16 ties of the
        # activations in a quarter of the outputs; the small variance is what makes eps visible)
        x = (rn(N, P, 256) * 2.0 ** -6).to(BF)
        s1 = (rn(Bi, 4 * P, 64) * 2.0 ** -6).to(BF)
        w0, b0 = rn(256, 256, scale=0.03).to(BF), torch.zeros(64)
        lw, lb = 1.5 + 0.1 * rn(64), 0.5 * rn(64)
    return dict(x=x, w0=w0, b0=b0, s1=s1, lw=lw, lb=lb, eps=1e-6, w1=w1, b1=b1, s0=s0, hyper=rn(N, 4, 32, scale=0.3).to(BF), es=es)


UPSCALE_TIGHT = 1e-4          # fp32 sums of 32 + 64 + 256 products of O(1) bf16 values and two erf GELUs (1.5e-7 each): a few 1e-6; x 10 of margin
UPSCALE_CAP = 1.6e-2          # elements behind a flipped bf16 tie of one of the 96 activations under an output: the CPU statement has 2e-4 .. 1.5e-3 of them
                              # (one flip moves up to 16 outputs: grainy on small cases, and it differs by a factor of two between CPUs); it must stay under a quarter of the cap


def upscale_check(d, name="", inst=None):
    """the two-level check of vg_mask_upscale against the float64 chain (tight: UPSCALE_TIGHT relative to the largest output, at least 1).  The wide
    bound has a floor, the size of one flipped tie: one bf16 ulp of the largest second-level activation times the largest |hyper| (the statement may
    happen to have no flipped tie at all on a small case, and then says nothing about their size); inst: the instances compared (large N)"""
    args = []
    ref = upscale_chain(d, F64, inst=inst, args=args)
    cpu = upscale_chain(d, F32, inst=inst)
    flip = float(R.quantum(gelu64(args[1]).abs().max(), BF)) * float(d["hyper"].float().abs().max())
    scale = ref.abs().max().clamp_min(1.0)
    return TwoLevel(name or "mask upscale", ref, torch.full_like(ref, UPSCALE_TIGHT) * scale, cpu, UPSCALE_CAP, flip)
