"""Exact-integer contraction tests (CPU only): generators, the float64 reference, poison / sentinel buffers, the failure diagnosis and the case
tables shared by tests/test_contraction_exact_gpu.py (the kernels) and tests/test_contraction_exact_selfcheck.py (the test's own power).

The idea: operands drawn from small integers ({-2, -1, 1, 2}: exact in bf16, e4m3 and e2m1 x 2^s).  Every product and every partial sum is then an
integer (a multiple of one power-of-two unit) far below 2^24, so an fp32 accumulation is exact in ANY order, split or tile walk: a kernel's
result must equal the float64 product bit for bit, and in bf16 that value's one round-to-nearest-even rounding.  No tolerance is chosen anywhere.
reference() proves the bound for every case it is given (the exactness guard) instead of assuming it."""
import torch

VALS = (-2, -1, 1, 2)
POISON = 2.0 ** 20            # exact in bf16 / fp32; one over-read element moves a sum of a few thousand out of any plausible range
SENTINEL = 7.0                # what an output buffer holds where the kernel must not write
LIMIT = 2.0 ** 24


def ints(shape, vals=VALS, seed=0):
    """float32 tensor of values drawn uniformly from `vals` (no zeros by default: every lost product shows)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(vals, dtype=torch.float32)
    return v[torch.randint(len(vals), tuple(shape), generator=g)]


def pow2(n, exps=(-1, 0, 1), seed=0):
    """float32 [n] of powers of two (LayerScale / norm weights / quantisation scales that keep every value on a power-of-two grid)"""
    return torch.ldexp(torch.ones(n), ints((n,), exps, seed).to(torch.int32))


def reference(x, w, bias=None, gamma=None, residual=None, relu=False, out_dtype=torch.float32, unit=1.0):
    """((relu?)(x @ w^T + bias)) * gamma + residual in float64, rounded ONCE to out_dtype.  `unit`: the grid the products live on (1 for integer
    operands; the product of the smallest scales for scaled ones).  The exactness guard: the largest sum of magnitudes any accumulation order can
    meet, epilogue operands included, counted in units, stays below 2^24 — so fp32 arithmetic is exact on this case in any order."""
    xd = x.double()
    acc, bound = [], []
    for n0 in range(0, w.shape[0], 512):                 # (row chunks of w: a 2000 x 32768 float64 copy would be 0.5 GB)
        wd = w[n0:n0 + 512].double()
        acc.append(xd @ wd.t())
        bound.append(xd.abs() @ wd.abs().t())
    acc, bound = torch.cat(acc, dim=1), torch.cat(bound, dim=1)
    if bias is not None:
        acc, bound = acc + bias.double(), bound + bias.double().abs()
    if relu:
        acc = acc.clamp_min(0.0)
    if gamma is not None:
        acc, bound = acc * gamma.double(), bound * gamma.double().abs()
        unit = unit * min(1.0, float(gamma.abs().min()))
    if residual is not None:
        acc, bound = acc + residual.double(), bound + residual.double().abs()
    assert float(bound.max()) / unit < LIMIT, f"not an exact case: {float(bound.max())} / {unit} >= 2^24"
    assert bool((torch.remainder(acc / unit, 1.0) == 0).all()), "the result is off the unit grid"
    y = acc.to(torch.float32)
    assert torch.equal(y.double(), acc)
    return y.to(out_dtype)


def poisoned(t, pad=16, guard=2, dtype=None, poison=POISON):
    """t [M, K] inside a larger [M + guard, K + pad] buffer whose gap columns and guard rows hold +poison / -2 poison alternately (no pair of
    neighbours cancels): returns the buffer; buffer[:M, :K] is the operand with a row stride K + pad.  Any read past K or past row M shows."""
    M, K = t.shape
    big = torch.empty(M + guard, K + pad, dtype=torch.float32)
    pat = torch.where((torch.arange(K + pad) % 2) == 0, poison, -2.0 * poison)
    big[:] = pat[None, :]
    big[1::2] *= -1.0
    big[:M, :K] = t
    return big.to(dtype or t.dtype)


def sentinel_out(M, N, dtype, device, pad=8, guard=1):
    """a SENTINEL-filled [guard + M + guard, pad + ceil8(N) + pad] buffer and the [M, N] view inside it that a kernel may write"""
    n8 = (N + 7) // 8 * 8
    big = torch.full((M + 2 * guard, n8 + 2 * pad), SENTINEL, dtype=dtype, device=device)
    return big, big[guard:guard + M, pad:pad + N]


def sentinel_intact(big, M, N, pad=8, guard=1):
    """True when nothing outside the [M, N] view of sentinel_out's buffer was written"""
    b = big.detach().float().cpu().clone()
    b[guard:guard + M, pad:pad + N] = SENTINEL
    return bool((b == SENTINEL).all())


def explain(got, want, x=None, w=None):
    """Where to read after a failure: the first wrong element, its error, the k whose product removed / doubled explains it, and the element's place
    in 64 / 128 / 256 tiles and 32 / 64 K steps.  x: [M, K], w: [N, K] as the kernel saw them (after any prologue)."""
    got, want = got.detach().double().cpu().reshape(want.shape), want.detach().double().cpu()
    bad = (got != want) | torch.isnan(got)
    if not bool(bad.any()):
        return "equal"
    want2, got2, bad2 = want.reshape(-1, want.shape[-1]), got.reshape(-1, want.shape[-1]), bad.reshape(-1, want.shape[-1])
    idx = bad2.nonzero()
    m, n = int(idx[0, 0]), int(idx[0, 1])
    d = float(got2[m, n] - want2[m, n])
    rows = sorted(set(idx[:, 0].tolist()))
    cols = sorted(set(idx[:, 1].tolist()))
    msg = [f"{int(bad.sum())} of {bad.numel()} wrong ({len(rows)} rows {rows[0]}..{rows[-1]}, {len(cols)} cols {cols[0]}..{cols[-1]}); first (m, n) = ({m}, {n}): "
           f"got {float(got2[m, n])!r} want {float(want2[m, n])!r} got - want = {d!r}"]
    for t in (64, 128, 256):
        msg.append(f"tile {t}: ({m // t}, {n // t}) + ({m % t}, {n % t})")
    if x is not None and w is not None and m < x.shape[0] and n < w.shape[0]:
        p = x[m].double().cpu() * w[n].double().cpu()
        for what, hit in (("removed", (p == -d)), ("doubled", (p == d))):
            ks = hit.nonzero().flatten().tolist()
            if ks:
                msg.append(f"one product {what} explains it at {len(ks)} k, e.g. k = {ks[:4]} .. {ks[-1]} (K step 32: {ks[-1] // 32}, 64: {ks[-1] // 64})")
        for step in (8, 32, 64):
            c = p.reshape(-1, step).sum(1) if p.numel() % step == 0 else None
            if c is not None:
                ks = (c == -d).nonzero().flatten().tolist()
                if ks:
                    msg.append(f"a dropped run of {step} k explains it at chunk(s) {ks[:4]} .. {ks[-1]} of {c.numel()}")
    return "; ".join(msg)


def check(got, want, x=None, w=None, what=""):
    """torch.equal with explain() as the message (and no NaN / inf: the poison is finite)"""
    g = got.detach().cpu()
    assert g.dtype == want.dtype and g.numel() == want.numel(), (what, g.dtype, want.dtype, tuple(g.shape), tuple(want.shape))
    assert torch.equal(g.reshape(want.shape), want), f"{what}: " + explain(g, want, x, w)


# ---- fp8 / MXFP4 operands built on the host (codes and power-of-two scales; no quantiser in the way)
def e4m3_codes(t):
    """uint8 OCP e4m3 codes of a tensor whose values are exactly representable (asserted)"""
    q = t.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), t.float())
    return q.view(torch.uint8)


_E2M1 = {0.0: 0, 0.5: 1, 1.0: 2, 1.5: 3, 2.0: 4, 3.0: 5, 4.0: 6, 6.0: 7}


def mxfp4_mean(elems, scales):
    """the float32 [N, K] matrix that e2m1 elements [N, K] with e8m0 scale bytes [N, K/32] mean to vg_decode_gemv_w4: block scale 2^(byte - 127), and a
    block whose scale byte is 0 contributes nothing (the kernel's documented reading of byte 0; the quantiser emits it for all-zero blocks only)"""
    N, nb = scales.shape
    sc = torch.where(scales == 0, torch.zeros(N, nb), torch.ldexp(torch.ones(N, nb), scales.to(torch.int32) - 127))
    return (elems.reshape(N, nb, 32) * sc[..., None]).reshape(N, -1)


def mxfp4_rows(N, K, seed=0):
    """logical MXFP4 rows of {-2, -1, 1, 2} elements: (codes uint8 [N, K/2], scales uint8 [N, K/32], the float32 [N, K] they mean, the unscaled
    elements [N, K]); every non-zero scale is >= 1, so the products stay on the integer grid.
    The block scales are 2^{0, 1, 2, 3} with neighbouring blocks ALWAYS different, and block 64 u + lane different from block 64 (u + 1) + lane (the
    packed head's walk); every row has 2^0 blocks, and one block per row (another one in every row) has the scale byte 0 under non-zero codes."""
    nb = K // 32
    elems = ints((N, K), VALS, seed)
    code = torch.where(elems.abs() == 1.0, 2, 4).to(torch.uint8) | ((elems < 0).to(torch.uint8) << 3)
    code = code.reshape(N, K // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).contiguous()
    b = torch.arange(nb)
    # exponent pattern: differs between b and b + 1 (parity bit) and between b and b + 64 (the 64-block bit), offset per row
    e = ((b % 2) + 2 * ((b // 64) % 2))[None, :].repeat(N, 1)
    e = (e + torch.arange(N)[:, None]) % 4
    scales = (e + 127).to(torch.uint8)
    assert bool((scales == 127).any(dim=1).all())
    scales[torch.arange(N), (torch.arange(N) * 7 + 3) % nb] = 0
    scales = scales.contiguous()
    assert bool((scales[:, 1:] != scales[:, :-1]).all()) and (nb <= 64 or bool((scales[:, 64:] != scales[:, :-64]).all()))
    return codes, scales, mxfp4_mean(elems, scales), elems


# ---- the blocked CPU GEMM model of the selfcheck (fp32 accumulation per K step, optional K split, one output rounding)
def model_gemm(x, w, kstep=64, ksplit=1, mutant=None, **kw):
    """x [M, K(+gap)], w [N, K(+gap)] float32 -> fp32 accumulator [M, N], K walked in steps of `kstep` inside `ksplit` slices whose partials are summed
    at the end, as the tile kernels and the split-K reduce do.  mutant: a name of MUTANTS (None = the honest kernel)."""
    K = kw.get("K", x.shape[1])
    nk = -(-K // kstep)
    per = -(-nk // ksplit)
    parts = []
    for z in range(ksplit):
        acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
        k0s = [s * kstep for s in range(z * per, min(nk, (z + 1) * per))]
        for k0 in k0s:
            k1 = min(K, k0 + kstep)
            xs, ws = x[:, k0:k1], w[:, k0:k1]
            if mutant == "last K element dropped" and k1 == K:
                xs, ws = xs[:, :-1], ws[:, :-1]
            if mutant == "last 8 K elements dropped" and k1 == K:
                xs, ws = xs[:, :-8], ws[:, :-8]
            if mutant == "one K step dropped" and k0 == (nk // 2) * kstep:
                continue
            if mutant == "x chunk i paired with w chunk i + 1" and k0 == (nk // 2) * kstep:
                n8 = (k1 - k0) // 8
                if n8 >= 2:
                    ws = torch.cat([ws[:, 8:8 * n8], ws[:, :8], ws[:, 8 * n8:]], dim=1)
                else:                                   # a single 8-element chunk: its neighbour is the previous chunk of the row
                    ws = w[:, k0 - 8:k1 - 8]
            if mutant == "lda gap read as data" and k1 == K:
                xs, ws = x[:, k0:k1 + 8], torch.cat([ws, torch.ones(w.shape[0], 8)], dim=1)      # (W read right, A runs 8 elements into its gap)
            acc = acc + xs @ ws.t()
            if mutant == "one K step counted twice" and k0 == (nk // 2) * kstep:
                acc = acc + xs @ ws.t()
        if mutant == "split-K boundary element counted by both slices" and z > 0 and k0s:
            b = k0s[0]
            acc = acc + x[:, b:b + 1] @ w[:, b:b + 1].t()
        if mutant == "a split-K slice dropped" and z == ksplit - 1 and ksplit > 1:
            continue
        parts.append(acc)
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def model_epilogue(acc, bias=None, gamma=None, residual=None, relu=False, out_dtype=torch.float32, mutant=None, tile=64):
    N = acc.shape[1]
    v = acc
    if bias is not None:
        b = bias.clone()
        if mutant == "bias missing in the last partial column group":
            b[(N - 1) // 8 * 8:] = 0.0
        v = v + b
    if relu:
        v = v.clamp_min(0.0)
    if gamma is not None:
        v = v * gamma
    if residual is not None:
        v = v + residual.float()
    if mutant == "an output tile shifted by one row":
        t0 = (acc.shape[0] - 1) // tile * tile             # the ragged last row tile
        v = v.clone()
        v[t0 + 1:] = v[t0:-1].clone()
    return v.to(out_dtype)


GEMM_MUTANTS = (
    "last K element dropped", "last 8 K elements dropped", "one K step dropped", "one K step counted twice",
    "split-K boundary element counted by both slices", "a split-K slice dropped", "x chunk i paired with w chunk i + 1",
    "an output tile shifted by one row", "bias missing in the last partial column group", "lda gap read as data",
)
MXFP4_MUTANTS = ("one MXFP4 block with its neighbour's scale", "packed MXFP4: the scale of block 64 u + lane taken from u + 1")
MUTANTS = GEMM_MUTANTS + MXFP4_MUTANTS


def mxfp4_mutant_weights(elems, scales, mutant):
    """the weights a kernel with a wrong scale walk would multiply by: elems [N, K] unscaled, scales [N, K/32] bytes"""
    nb = scales.shape[1]
    s2 = scales.clone()
    if mutant == MXFP4_MUTANTS[0]:
        s2[:, nb // 2] = scales[:, nb // 2 + 1]
    elif mutant == MXFP4_MUTANTS[1]:
        lane = 5
        s2[:, lane] = scales[:, 64 + lane]             # u = 0 reads u = 1's byte
    return mxfp4_mean(elems, s2)


# ---- the cases (shared by the GPU tests and the selfcheck)
# ops.linear: (route, env, [(M, N, K), ...]); route codes of vg_gemm_route
_K64B = [(M, N, K) for M, N in ((17, 40), (129, 136), (300, 200)) for K in (72, 144, 200, 328)]
LINEAR_ROUTES = {
    "skinny": (0, {}, [(M, N, K) for M in (1, 3, 4, 5, 8, 9, 16) for N in (33, 512) for K in (8, 72, 2048, 14336)]),
    "k64b": (2, {"VG_GEMM_SPLITK": "0"}, _K64B),
    "small64": (5, {}, [(65, 64, 64), (300, 72, 192), (129, 200, 256)]),
    "s128": (4, {"VG_GEMM_SPLITK": "0"}, [(300, 200, 520), (129, 72, 1536)]),      # (fp32 at K = 1536 would be split-K by ops.linear's rule)
    "glds": (1, {"VG_GEMM_SPLITK": "0"}, [(129, 130, 1544), (257, 136, 4160)]),
    # (VG_GEMM_SPLITK=0 with the forced routes too: ops.linear's split-K rule comes before vg_gemm and would take the few-tile long-K shapes)
    "p8": (3, {"VG_GEMM_P8": "2", "VG_GEMM_SPLITK": "0"}, [(300, 264, 576), (513, 520, 704), (257, 256, 4160)]),
    "p8n": (6, {"VG_GEMM_P8": "3", "VG_GEMM_SPLITK": "0"}, [(4111, 1160, 128), (777, 384, 320), (300, 192, 4096)]),
    "rr": (7, {"VG_GEMM_RR": "2"}, [(300, 144, 144), (1000, 432, 288)]),
}
SPLITK = [(M, N, K, ks) for (M, N, K) in ((40, 136, 4160), (213, 264, 14336)) for ks in (2, 3, 4, 8)]
WINDOWS = [(1, 20, 12, 7, 72, 40), (2, 16, 16, 8, 144, 432)]           # (B, H, W, ws, K, N)
BMM = [(3, 70, 50, 64), (3, 4, 1000, 32), (2, 3, 4133, 32), (2, 129, 136, 72)]      # (B, M, N, K); the middle two with fp32 output
BMM_SHARED = (40, 136, 72)
QKV = [(16, 2, 128, 2048), (16, 2, 128, 4096)]                       # (H, Hkv, D, K)


def fp32_tile_route(K):
    """the fp32 route of an M > 16 GEMM (vg_gemm.hip's rule restated: rows of K x 4 bytes up to 3 KB take the short-K kernels, from 1 KB the
    128-byte-row one; fp32 has no 256-row tile, small-problem or row-register kernel)"""
    return (4 if K * 4 >= 1024 else 2) if K * 4 <= 3072 else 1
F8 = [(130, 264, 144), (200, 512, 256), (33, 136, 4096)]
GEMV_N = (33, 257, 1001)
GEMV_K = (64, 176, 2048, 3072, 4096, 8192, 14336, 32768)
GEMV_Q_N = (33, 1001)
GEMV_Q_K = (3072, 4096, 8192, 14336)
ROWS_B = (1, 3, 16)
ROWS_K = (2048, 3072, 14336)
W8_ROWS_B = (1, 5, 16)
MLP3 = [(G, R, K, Hd, No) for G in (1, 2, 4) for R in (1, 33) for (K, Hd, No) in ((16, 16, 1), (256, 256, 4), (256, 256, 32))]
LINEAR_ROWS = [(M, N, K) for K in (64, 128, 192, 256) for N in (64, 192) for M in (150,)]      # 150 = 2 x 64 + 22: a ragged last block


def epilogue_operands(M, N, seed, res_dtype=torch.bfloat16):
    """integer fp32 bias, power-of-two gamma, integer residual (|r| <= 8: exact in bf16 whatever it is added to within the guard)"""
    return ints((N,), (-3, -1, 2, 5), seed + 1), pow2(N, (-1, 0, 1), seed + 2), ints((M, N), (-8, -3, 1, 6), seed + 3).to(res_dtype)
