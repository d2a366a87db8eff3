"""Plain-torch side of the row-wise accuracy tests: norms, norm prologues, activations and rotations against float64 at rounding level (CPU only).

Shared by tests/test_rowwise_accuracy_gpu.py (the kernels) and tests/test_rowwise_accuracy_selfcheck.py (the test's own power).  For every case, on
the exact stored operands:

  ref64   the statement of tests/_cpu_ops.py in float64 with exactly the intermediate roundings the kernels document (bf16 RMSNorm rounds x * rstd
          to bf16 before the weight, bf16 SwiGLU rounds silu(gate) to bf16 before the product, bf16 rope_half rounds cos, sin and every product);
          nothing else is rounded before the end.
  model   ref64 rounded once, to nearest even, to the output dtype (round_to: straight from float64, no double rounding through fp32).
  element |got - ref64| <= 1/2 ulp_out(ref64) + slack,  slack = fixed + mult * unit.  `unit` is the closed form of the fp32 arithmetic of the family
          (below, in units of 2^-24), `fixed` a documented approximation error that no multiple scales, and `mult` = max(4, 4 x the largest multiple
          the CPU fp32 statement itself needs against ref64 on the same inputs) — measured here on the CPU, never from a kernel.  The factor four
          is for what torch's CPU code does not have: another summation tree and the 1-ulp v_rsq / v_rcp / v_exp.  Families whose closed form is
          a worst case of the arithmetic (axial / half RoPE in fp32, axpby) carry a fixed multiple of 2 and measure nothing.
  share   (bf16 outputs) the share of elements with got != model is at most max(4 x the share of the CPU fp32 statement rounded to bf16, 1e-3);
          the statement's own share must be <= 2.5e-4 (asserted before a kernel is looked at: a condition on the inputs).

The closed forms (y: the float64 result, U = 2^-24):
  LayerNorm   unit = U ((|x| + |mean|) rstd |w| + |y|).  The first term is the cancellation in x - mean (mean carries a few ulps of its own
              magnitude; the difference inherits them in absolute terms, scaled by rstd |w|), and the rounding of the product n * w; the second
              the final addition of b.  An output near zero may therefore sit several of its own ulps away in an honest fp32 kernel.
  RMSNorm     unit = U (|x| rstd |w| + |y|)  (no mean).
  erf GELU    fixed = 0.75e-7 |x| (Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7, halved in Phi), unit = U |x| (Phi <= 1, a handful of fp32
              operations on values <= 1 before the final product with x).
  x sigma(z), sigma(z)   (SiLU z = x, quick-GELU z = 1.702 x, sigmoid)  unit = U |y| (1 + |z| sigma(-z)): v_exp_f32 and v_rcp_f32 are 1 ulp each and
              1 + e one rounding — relative errors of y; the argument of exp is rounded once, which moves exp(-z) by |z| U relatively and y by
              y sigma(-z) |z| U.  fixed = 2^-126 max(1, |x|): the fast exp / rcp flush results below the smallest normal fp32.
  SwiGLU      the SiLU form times |u|, plus U |y| for the product.
  axial RoPE, fp32 half RoPE, axpby   2 U (|p| + |q|) for y = p +- q, p and q products: fl(p) + fl(q) + the sum, or one product and an FMA.
  sigmoid mask  (vg_mask_for_mem, sigmoid mode: IEEE expf and division)  unit = U (|s scale| (1 + |x| sigma(-x)) + |y|).

Ambiguous intermediate roundings: where the float64 value that is rounded to bf16 inside the statement (x * rstd, silu(gate)) lies within
TIE x 2^-24 (relative) of the midpoint of two bf16 numbers, an honest fp32 kernel may land on either side, one bf16 ulp apart.  ref64 then exists in
both versions and an element passes when it meets the bound for either (about 2 TIE 2^-24 / 2^-8 = 5e-4 of the elements are in that position; a kernel
that skips the rounding differs on a third of ALL elements).  The share check counts an element as a mismatch when it equals the model of neither version:
bf16 inputs take few distinct values, a row's x * rstd repeats with them, and one value next to a tie would move dozens of elements at once.

Probe rows (build_norm_rounds): besides the random rows N(3, 1), at most a quarter of the rows (at least one) carry
  spike   one 8-sigma spike at the first column, the last column, the first column of the last 16-byte chunk, and the first and last column of each
          pass j of the per-lane chunk walk (columns j TPR NV and min((j + 1) TPR NV, C) - 1 of the route the case is meant for);
  offset  mean 64 (bf16) / 1000 (fp32) at unit variance: a one-pass variance in fp32 shows in the fp32 outputs;
  step    (bf16) 256 everywhere but 258 in every 64th column and the last: mean / sigma = 1000, a one-pass variance shows in bf16 outputs too;
  quiet   sigma = 2^-6 (about 3 for LayerNorm, about 0 for RMSNorm): the variance is comparable with 100 eps, a wrong eps shows grossly;
  const   a constant row: variance 0, LayerNorm's output is b up to the rounding of the mean.
What does not fit a quarter of the rows goes to later rounds of the same case (rows = 3 or 5), as the attention test does.  The offset, step, quiet
and const rows are built so that x - mean cancels: there the fp32 statement itself sits several output roundings from float64 (a third of a step
row's elements in torch's own LayerNorm), so the share check does not count them, as it does not count GELU below -1; the element check, whose
first term is that cancellation, covers them.  The spike rows are counted.  Where the power then comes from: on the offset, step, quiet and const
rows (step and quiet are additions of this helper, not of the issue's list), and for a case without weights, whose share counts each distinct value
of a row once, the ELEMENT check alone carries the power — eps x 10 without weights moves the share to 4e-4 .. 1e-3 only, below the cap, and fails
through the quiet row's elements; the statistics mutants fail through the element check on the spike rows in every shape class (self-check).
"""
import math

import torch
import torch.nn.functional as F

BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
TIE = 16.0                    # see "ambiguous intermediate roundings"
FLOOR = 4.0                   # the floor of a measured multiple
FACTOR = 4.0                  # kernel multiple / CPU statement multiple
SHARE_FLOOR = 1e-3
SHARE_CPU_MAX = 2.5e-4
ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_SILU, ACT_SIGMOID = 1, 2, 3, 4, 5
UNCOUNTED = ("offset", "step", "quiet", "const")
QUICK = float(torch.tensor(1.702, dtype=F32))          # the constant as the kernels hold it


# ------------------------------------------------------------------ formats
def quantum(v, dtype):
    """float64 tensor: the spacing of `dtype` in the binade of |v| (subnormal spacing below the smallest normal)"""
    p = 8 if dtype == BF else 24
    v = v.abs()
    _, e = torch.frexp(v)                                   # |v| in [2^(e - 1), 2^e)
    e = torch.where(v == 0, torch.full_like(e, -125), e).clamp(min=-125)
    return torch.exp2(e.double() - p)


def round_to(v, dtype):
    """float64 -> dtype, ONE rounding to nearest even (v / quantum is exact; torch.round rounds halves to even)"""
    q = quantum(v, dtype)
    return (torch.round(v / q) * q).to(dtype)


def rbf(v):
    """float64 -> the float64 value of its bf16 rounding"""
    return round_to(v, BF).double()


# ------------------------------------------------------------------ a case and its checks
class Case:
    """refs / units: the versions of ref64 (see the module docstring) and their units; fixed: the part of the slack no multiple scales;
    cpu32: the CPU fp32 statement's output in fp32 (None: no share check); fixed_mult: a multiple that is a worst case of the arithmetic (nothing is
    measured); counted: bool mask of the elements the share check counts (None: all)."""

    def __init__(self, name, refs, units, out_dtype, cpu32=None, fixed=None, fixed_mult=None, counted=None, route=""):
        self.name, self.refs, self.units, self.out_dtype, self.cpu32 = name, refs, units, out_dtype, cpu32
        self.fixed = fixed if fixed is not None else torch.zeros_like(refs[0])
        self.fixed_mult, self.counted, self.route = fixed_mult, counted, route
        self._mult, self._models = None, None

    def need(self, got, dtype, mult=FLOOR):
        """float64 tensor: the multiple of `unit` every element of `got` (a tensor of `dtype`) needs, best version (inf: not finite); mult: the
        multiple allowed (it only decides which binade's 1/2 ulp an element next to a power of two is entitled to)"""
        g = got.double().reshape(self.refs[0].shape)
        best = torch.full_like(g, float("inf"))
        for ref, unit in zip(self.refs, self.units):
            err = (g - ref).abs()
            # 1/2 ulp of the binade the honest fp32 value can lie in: ref64's, or its neighbour's when the slack crosses a power of two
            excess = (err - 0.5 * quantum(ref.abs() + self.fixed + mult * unit, dtype) - self.fixed).clamp_min(0.0)
            n = torch.where(excess == 0, torch.zeros_like(excess), excess / unit.clamp_min(1e-300))
            best = torch.minimum(best, torch.where(torch.isfinite(g), n, torch.full_like(n, float("inf"))))
        return best

    def mult(self):
        """(the multiple a kernel is allowed, the multiple the CPU fp32 statement needs)"""
        if self._mult is None:
            if self.fixed_mult is not None:
                self._mult = (self.fixed_mult, 0.0)
            else:
                cpu = float(self.need(self.cpu32, F32).max())
                assert math.isfinite(cpu), self.name
                self._mult = (max(FLOOR, FACTOR * cpu), cpu)
        return self._mult

    def model(self):
        return round_to(self.refs[0], self.out_dtype)

    def _mismatch(self, t):
        """bool: t differs from the model in EVERY version of ref64 (an element whose intermediate rounding is ambiguous may take either)"""
        if self._models is None:
            self._models = [round_to(r, self.out_dtype) for r in self.refs]
        t = t.reshape(self.refs[0].shape)
        bad = t != self._models[0]
        for m in self._models[1:]:
            bad &= t != m
        return bad

    def shares(self, got):
        """(share of got != model, share of the CPU statement rounded to the output dtype, the cap) over the counted elements"""
        sel = self.counted if self.counted is not None else torch.ones_like(self.refs[0], dtype=torch.bool)
        n = max(1, int(sel.sum()))
        sk = float((self._mismatch(got) & sel).sum()) / n
        sc = float((self._mismatch(self.cpu32.to(self.out_dtype)) & sel).sum()) / n
        return sk, sc, max(FACTOR * sc, SHARE_FLOOR)

    def precondition(self):
        """the condition on the inputs the share cap rests on (CPU only)"""
        if self.out_dtype == BF and self.cpu32 is not None:
            sc = self.shares(self.model())[1]
            assert sc <= SHARE_CPU_MAX, f"{self.name}: the fp32 statement's own share {sc:.2e} > {SHARE_CPU_MAX:.1e}: not a case for the share check"

    def evaluate(self, got):
        """-> dict(ok, need, mult, cpu, share, share_cpu, cap, bad): the element check and (bf16 outputs with a statement) the share check"""
        assert got.dtype == self.out_dtype, (self.name, got.dtype, self.out_dtype)
        got = got.detach().cpu()
        mult, cpu = self.mult()
        need = self.need(got, self.out_dtype, mult)
        worst = float(need.max())
        r = dict(need=worst, mult=mult, cpu=cpu, share=0.0, share_cpu=0.0, cap=0.0, bad=int((need > mult).sum()))
        ok = worst <= mult
        if self.out_dtype == BF and self.cpu32 is not None:
            r["share"], r["share_cpu"], r["cap"] = self.shares(got)
            ok = ok and r["share"] <= r["cap"]
        r["ok"] = bool(ok)
        return r


def line(case, r):
    return (f"ACC {case.name:58s} route {case.route:22s} need {r['need']:8.2f} of {r['mult']:6.2f} (cpu {r['cpu']:5.2f}) "
            f"share {r['share']:.2e} cap {r['cap']:.2e} (cpu {r['share_cpu']:.2e})")


def check(case, got, precondition=True):
    """the assertion of the GPU tests (prints the ACC line first)"""
    if precondition:
        case.precondition()
    r = case.evaluate(got)
    print(line(case, r))
    if not r["ok"]:
        need = case.need(got.detach().cpu(), case.out_dtype)
        i = int(need.reshape(-1).argmax())
        where = [int(v) for v in torch.unravel_index(torch.tensor(i), need.shape)]
        raise AssertionError(f"{case.name}: {r['bad']} elements over the bound, worst at {where}: got {float(got.detach().cpu().double().reshape(-1)[i])!r} "
                             f"ref64 {float(case.refs[0].reshape(-1)[i])!r} needs {r['need']:.2f} units of {r['mult']:.2f}; share {r['share']:.3e} cap {r['cap']:.3e}")
    return r


# ------------------------------------------------------------------ norms
def norm_case(name, x, w, b, eps, rms, out_dtype, route="", probes=None):
    """x [rows, C] as stored (bf16 / fp32), w / b fp32 [C] or None; probes: {row: kind} of build_norm_rounds (the cancellation rows are not counted
    by the share check: module docstring)"""
    xd = x.double()
    C = x.shape[-1]
    wd = w.double() if w is not None else torch.ones(C, dtype=torch.float64)
    bd = b.double() if b is not None else torch.zeros(C, dtype=torch.float64)
    if rms:
        assert b is None
        rstd = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps)
        n = xd * rstd
        ns = [n]
        if x.dtype == BF:          # the reference model rounds the normalised value to the activation dtype before the weight
            d = TIE * U * n.abs()
            ns = [rbf(n), rbf(n - d), rbf(n + d)]
        refs = [v * wd for v in ns]
        units = [U * (xd.abs() * rstd * wd.abs() + r.abs()) for r in refs]
        y = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype).float()          # _cpu_ops.rmsnorm, fp32 output
        cpu32 = y * w if w is not None else y
    else:
        mean = xd.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + eps)
        y = (xd - mean) * rstd * wd + bd
        refs = [y]
        units = [U * ((xd.abs() + mean.abs()) * rstd * wd.abs() + y.abs())]
        cpu32 = F.layer_norm(x.float(), (C,), w, b, eps)                                                       # _cpu_ops.layernorm, fp32 output
    counted = torch.ones(x.shape, dtype=torch.bool)
    if w is None and b is None:
        # no per-column operand: columns of a row that hold the same x are ONE computation repeated (a bf16 row of N(3, 1) has about 300 distinct
        # values), and one value next to a tie would count dozens of times: the share counts each distinct value of a row once
        xs, order = x.float().sort(dim=1, stable=True)
        first = torch.cat([torch.ones(x.shape[0], 1, dtype=torch.bool), xs[:, 1:] != xs[:, :-1]], dim=1)
        counted = torch.zeros(x.shape, dtype=torch.bool).scatter_(1, order, first)
    for row, kind in (probes or {}).items():
        if kind in UNCOUNTED:
            counted[row] = False
    return Case(name, refs, units, out_dtype, cpu32=cpu32, counted=counted, route=route)


def spike_columns(C, tpr, nv):
    """the columns a dropped / doubled column of the chunk walk (t + j TPR) NV < C would be: module docstring"""
    cols = [0, C - 1, max(0, (C - 1) // nv * nv)]
    step = tpr * nv
    for j in range(-(-C // step)):
        cols += [j * step, min((j + 1) * step, C) - 1]
    return sorted(set(cols))


def _probe_row(kind, C, dtype, rms, g):
    if kind == "offset":
        return (64.0 if dtype == BF else 1000.0) + torch.randn(C, generator=g)
    if kind == "step":
        r = torch.full((C,), 256.0)
        r[63::64] = 258.0
        r[C - 1] = 258.0
        return r
    if kind == "quiet":
        return (0.0 if rms else 3.0) + 2.0 ** -6 * torch.randn(C, generator=g)
    if kind == "const":
        return torch.full((C,), 3.0)
    r = 3.0 + torch.randn(C, generator=g)
    r[kind] = 3.0 + 8.0          # a spike row: kind is the column
    return r


def build_norm_rounds(rows, C, dtype, rms, tpr, nv, seed=0):
    """[(x [rows, C] of dtype, probe rows {row: kind})]: random rows N(3, 1) with the probe rows (module docstring) as the LAST rows of every round"""
    kinds = list(spike_columns(C, tpr, nv)) + ["offset", "quiet", "const"] + (["step"] if dtype == BF and C >= 64 else [])
    cap = max(1, rows // 4)
    out = []
    if rows == 1:          # a one-row case (a decode step): one round of its own for the random row
        out.append(((3.0 + torch.randn(1, C, generator=torch.Generator().manual_seed(1000 * seed + C + 5))).to(dtype), {}))
    for r0 in range(0, len(kinds), cap):
        g = torch.Generator().manual_seed(1000 * seed + 7 * rows + C + r0)
        x = 3.0 + torch.randn(rows, C, generator=g)
        mine = kinds[r0:r0 + cap]
        probes = {}
        for i, kind in enumerate(mine):
            row = rows - len(mine) + i
            x[row] = _probe_row(kind, C, dtype, rms, g)
            probes[row] = kind
        out.append((x.to(dtype), probes))
    return out


def cat_cases(name, cases):
    """the rounds of one case as one (element and share checks over all rounds together)"""
    c0 = cases[0]
    nv = len(c0.refs)
    pick = lambda f: torch.cat([f(c).reshape(-1) for c in cases])          # noqa: E731
    return Case(name, [pick(lambda c, i=i: c.refs[i]) for i in range(nv)], [pick(lambda c, i=i: c.units[i]) for i in range(nv)], c0.out_dtype,
                cpu32=pick(lambda c: c.cpu32) if c0.cpu32 is not None else None, fixed=pick(lambda c: c.fixed), fixed_mult=c0.fixed_mult,
                counted=pick(lambda c: c.counted) if c0.counted is not None else None, route=c0.route)


def mlp_onehot_case(name, x, lw, lb, eps, probes, route=""):
    """vg_mlp_rows under w1 = identity blocks (zero bias) and a one-hot w2 whose four hidden copies carry 0.25 each (exact):
    y = x + bf16(gelu(bf16(LayerNorm(x)))) in bf16.  Both intermediate roundings are ambiguous within the slack of the stage before them (the
    LayerNorm's and the GELU's own bounds, multiples measured from their CPU statements), so ref64 exists in 3 x 3 versions; the last stage is one
    fp32 sum of two bf16 numbers and the zero bias (2 U |y|)."""
    ln = norm_case(name, x, lw, lb, eps, False, BF)
    d = ln.mult()[0] * ln.units[0]
    refs = []
    for n in (rbf(ln.refs[0]), rbf(ln.refs[0] - d), rbf(ln.refs[0] + d)):
        g, unit, fixed, _ = act_ref(n, ACT_GELU)
        s = fixed + act_case(name, n.to(BF), ACT_GELU, BF).mult()[0] * unit
        refs += [x.double() + h for h in (rbf(g), rbf(g - s), rbf(g + s))]
    h32 = F.gelu(F.layer_norm(x.float(), (x.shape[-1],), lw, lb, eps).to(BF).float()).to(BF).float()          # _cpu_ops.mlp_rows with these weights
    counted = torch.ones(x.shape, dtype=torch.bool)
    for row, kind in (probes or {}).items():
        if kind in UNCOUNTED:
            counted[row] = False
    return Case(name, refs, [U * r.abs() for r in refs], BF, cpu32=x.float() + h32, fixed_mult=2.0, counted=counted, route=route)


def norm_weights(C, seed=0):
    g = torch.Generator().manual_seed(77 + seed + C)
    return torch.randn(C, generator=g), torch.randn(C, generator=g)


# ------------------------------------------------------------------ activations
def act_grid(dtype):
    """a grid over [-12, 12] plus +-0, +-20, +-88, +-100 and the largest finite bf16, in `dtype` (a multiple of 8 elements).  fp32: 24 000 evenly
    spaced points.  bf16: EVERY bf16 number with 2^-16 <= |x| <= 12, each once (about 5000: evenly spaced points rounded to bf16 repeat each of
    1900 numbers a dozen times, and one number next to a tie would then count a dozen times in the share)."""
    big = float(torch.finfo(BF).max)
    pts = torch.tensor([0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, big, -big, 2.0 ** -20, -2.0 ** -20])
    if dtype == BF:
        allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF).float()
        grid = allv[torch.isfinite(allv) & (allv.abs() >= 2.0 ** -16) & (allv.abs() <= 12.0)]
    else:
        grid = torch.linspace(-12.0, 12.0, 24000)
    out = torch.cat([grid, pts])
    return torch.cat([out, torch.ones(-out.numel() % 8)]).to(dtype)


def _sig(z):
    return torch.sigmoid(z)


def act_ref(x, act):
    """(ref64, unit, fixed, counted) of activation `act` on the stored x"""
    xd = x.double()
    counted = None
    if act == ACT_GELU:
        y = xd * 0.5 * torch.special.erfc(-xd / math.sqrt(2.0))
        unit, fixed = U * xd.abs(), 0.75e-7 * xd.abs()
        counted = xd >= -1.0          # below, 0.5 - q cancels by design (vg_common.h): the element check covers that tail
    elif act == ACT_RELU:
        y = xd.clamp_min(0.0)
        unit, fixed = torch.zeros_like(xd), torch.zeros_like(xd)
    else:
        z = xd * QUICK if act == ACT_QUICK_GELU else xd
        s = _sig(z)
        y = s if act == ACT_SIGMOID else xd * s
        unit = U * y.abs() * (1.0 + z.abs() * _sig(-z))
        unit = torch.where(torch.isfinite(unit), unit, torch.zeros_like(unit))
        fixed = FLT_MIN * xd.abs().clamp_min(1.0)
    return y, unit, fixed, counted


def act_cpu32(x, act):
    """tests/_cpu_ops.py: _act in fp32"""
    xf = x.float()
    if act == ACT_GELU:
        return F.gelu(xf)
    if act == ACT_QUICK_GELU:
        return xf * torch.sigmoid(1.702 * xf)
    if act == ACT_RELU:
        return F.relu(xf)
    if act == ACT_SILU:
        return F.silu(xf)
    return torch.sigmoid(xf)


def act_case(name, x, act, out_dtype, route=""):
    y, unit, fixed, counted = act_ref(x, act)
    cpu = act_cpu32(x, act)
    # (torch's fp32 GELU overflows at the largest finite bf16, where x Phi(x) = x is finite: the statement stands aside on such a point)
    cpu = torch.where(torch.isfinite(cpu), cpu, y.float())
    return Case(name, [y], [unit], out_dtype, cpu32=cpu, fixed=fixed, counted=counted, route=route)


def swiglu_case(name, gu, route=""):
    """gu [M, 2 F] as stored: silu(gate) (rounded to bf16 in bf16) times up"""
    Fh = gu.shape[-1] // 2
    g, u = gu[..., :Fh].double(), gu[..., Fh:].double()
    s, sunit, sfixed, _ = act_ref(gu[..., :Fh], ACT_SILU)
    ss = [s]
    if gu.dtype == BF:
        d = TIE * sunit
        ss = [rbf(s), rbf(s - d), rbf(s + d)]
    refs = [v * u for v in ss]
    units = [sunit * u.abs() + U * r.abs() for r in refs]
    sil = F.silu(gu[..., :Fh].float()).to(gu.dtype).float()
    return Case(name, refs, units, gu.dtype, cpu32=sil * gu[..., Fh:].float(), fixed=sfixed * u.abs(), route=route)


def two_product_case(name, p, q, out_dtype, route="", cpu32=None):
    """y = p + q with p, q float64 products of stored operands: 2 U (|p| + |q|), no measured multiple (cpu32: the statement, for the share check)"""
    return Case(name, [p + q], [U * (p.abs() + q.abs())], out_dtype, cpu32=cpu32, fixed_mult=2.0, route=route)


def axpby_case(name, a, b, alpha, beta, out_dtype, route=""):
    al, be = float(torch.tensor(alpha, dtype=F32)), float(torch.tensor(beta, dtype=F32))
    ad = a.double()
    # (element check only: a bf16 a plus a short multiple of a bf16 b lands on or next to a bf16 tie in percents of the elements, where the one
    # rounding of the model and the fp32-then-bf16 rounding of any fp32 kernel legitimately part; the share of such a case says nothing)
    if b is None:
        return two_product_case(name, al * ad, torch.full_like(ad, be), out_dtype, route)
    bb = b.reshape(-1).repeat(a.numel() // b.numel()).reshape(a.shape)
    return two_product_case(name, al * ad, be * bb.double(), out_dtype, route)


def mask_sigmoid_case(name, x, scale, bias, out_dtype, route=""):
    xd = x.double()
    sc, bi = float(torch.tensor(scale, dtype=F32)), float(torch.tensor(bias, dtype=F32))
    s = _sig(xd)
    y = s * sc + bi
    unit = U * ((s * sc).abs() * (1.0 + xd.abs() * _sig(-xd)) + y.abs())
    return Case(name, [y], [unit], out_dtype, cpu32=torch.sigmoid(x.float()) * scale + bias, fixed=torch.full_like(xd, FLT_MIN * abs(sc)),
                route=route)


# ------------------------------------------------------------------ rotations
def rope_half_bf16(x, cos, sin, pos0, flip_sin_half=False, fp32_products=False):
    """the fully specified bf16 arithmetic of vg_rope_half / vg_rope_kv_append on x [S, H, D] bf16 (returns a new tensor): cos / sin rounded to
    bf16, every product rounded to bf16 (a bf16 x bf16 product is exact in fp32, so the rounding is the only one), the sum of two bf16 numbers in
    fp32 rounded to bf16.  The keyword arguments are the self-check's wrong kernels."""
    S, H, D = x.shape
    c = cos[pos0:pos0 + S].to(BF).float()[:, None, :]
    s = sin[pos0:pos0 + S].to(BF).float()[:, None, :]
    x1, x2 = x[..., : D // 2].float(), x[..., D // 2:].float()
    r = (lambda t: t) if fp32_products else (lambda t: t.to(BF).float())
    o1 = r(x1 * c) + r(-x2 * s)
    o2 = r(x2 * c) + (r(-x1 * s) if flip_sin_half else r(x1 * s))
    return torch.cat([o1, o2], dim=-1).to(BF)


def rope_half_case(name, x, cos, sin, pos0):
    """fp32 x [S, H, D]: the element check"""
    S, H, D = x.shape
    c, s = cos[pos0:pos0 + S].double()[:, None, :], sin[pos0:pos0 + S].double()[:, None, :]
    x1, x2 = x[..., : D // 2].double(), x[..., D // 2:].double()
    p = torch.cat([x1 * c, x2 * c], dim=-1)
    q = torch.cat([-x2 * s, x1 * s], dim=-1)
    return two_product_case(name, p, q, x.dtype, "rope_half_kernel")


def rope_axial_case(name, x, cos, sin, n_rope, n_grid, route=""):
    """x [B, N, C] as stored; the first n_rope tokens rotated by the table row tok % n_grid; returns (case over the rotated tokens)"""
    B, N, C = x.shape
    xr = x[:, :n_rope].double().reshape(B, n_rope, C // 2, 2)
    idx = torch.arange(n_rope) % n_grid
    c, s = cos.double()[idx][None], sin.double()[idx][None]
    a, b = xr[..., 0], xr[..., 1]
    p = torch.stack([a * c, a * s], dim=-1).reshape(B, n_rope, C)
    q = torch.stack([-b * s, b * c], dim=-1).reshape(B, n_rope, C)
    return two_product_case(name, p, q, x.dtype, route, rope_axial_fp32(x, cos, sin, n_rope, n_grid))


# ------------------------------------------------------------------ honest transcriptions and wrong kernels (the self-check's stand-ins)
def _butterfly(v):
    """group_sum: xor butterfly over the last dim (a power of two), widest step first, fp32"""
    n = v.shape[-1]
    step = n // 2
    idx = torch.arange(n)
    while step >= 1:
        v = v + v[..., idx ^ step]
        step //= 2
    return v[..., 0]


def norm_lanes_fp32(x, w, b, eps, rms, tpr, nv=8, mutant=None):
    """norm_short_kernel / norm_kernel's register path in fp32 torch: lane t of TPR sums its chunks (t + j TPR) NV .. + NV - 1 in order, pairs first
    as the kernel adds them, the lanes are reduced by the butterfly, mean = sum * (1 / C), two-pass variance, y = (x - mean) rstd w + b.
    mutant: one of NORM_MUTANTS (None: the honest kernel).  Returns fp32 [rows, C]."""
    rows, C = x.shape
    step = tpr * nv
    nj = -(-C // step)
    xf = x.float()
    live = torch.ones(C, dtype=torch.bool)          # the columns that enter the statistics
    weight = torch.ones(C)
    div = float(C)
    if mutant == "last column dropped from the statistics":
        live[C - 1] = False
    elif mutant == "last 8-column chunk dropped":
        live[(C - 1) // nv * nv:] = False
    elif mutant == "one column counted twice":
        weight[min(C - 1, step)] = 2.0          # the first column of the second pass (the last column when there is one pass)
    elif mutant == "divisor C - 1":
        div = float(C - 1)
    elif mutant == "divisor padded to the lane width":
        div = float(nj * step)
    epsv = eps * 10.0 if mutant == "eps x 10" else eps
    inv = torch.tensor(1.0 / div, dtype=F32)

    def lanes(v):          # [rows, C] -> [rows] by the kernel's walk
        pad = torch.zeros(rows, nj * step, dtype=F32)
        pad[:, :C] = v * (live.float() * weight)
        acc = torch.zeros(rows, tpr, dtype=F32)
        if nv == 1:          # the scalar walk: c = t, t + TPR, ...
            for j in range(nj):
                acc = acc + pad.reshape(rows, nj, tpr)[:, j]
            return _butterfly(acc)
        pad = pad.reshape(rows, nj, tpr, nv // 2, 2)
        for j in range(nj):
            for e in range(nv // 2):
                acc = acc + (pad[:, j, :, e, 0] + pad[:, j, :, e, 1])
        return _butterfly(acc)
    if rms and mutant != "RMSNorm that subtracts a mean":
        mean = torch.zeros(rows, 1)
    else:
        mean = (lanes(xf) * inv)[:, None]
    if mutant == "one-pass fp32 variance":
        var = (lanes(xf * xf) * inv)[:, None] - mean * mean
    else:
        d = xf - mean
        var = (lanes(d * d) * inv)[:, None]
    rstd = torch.rsqrt(var + torch.tensor(epsv, dtype=F32))
    n = (xf - mean) * rstd
    if rms:
        if x.dtype == BF and mutant != "RMSNorm without the intermediate rounding":
            n = n.to(BF).float()
        return n * w if w is not None else n
    y = n * (w if w is not None else 1.0)
    if b is not None:
        bb = b.clone()
        if mutant == "LayerNorm that forgets b on the last chunk":
            bb[(C - 1) // nv * nv:] = 0.0
        y = y + bb
    return y


NORM_MUTANTS = ("last column dropped from the statistics", "last 8-column chunk dropped", "one column counted twice", "divisor C - 1",
                "divisor padded to the lane width", "one-pass fp32 variance", "eps x 10")
RMS_MUTANTS = ("RMSNorm without the intermediate rounding", "RMSNorm that subtracts a mean")
LN_MUTANTS = ("LayerNorm that forgets b on the last chunk",)


def gelu_device_fp32(x):
    """vg_gelu_erf (vg_common.h) in fp32 torch: the same constants and order; the FMAs as a product and a sum, v_rcp / v_exp2 as torch's"""
    f = lambda v: torch.tensor(v, dtype=F32)          # noqa: E731
    x = x.float()
    a = x.abs()
    t = 1.0 / (f(0.3275911 * 0.70710678118654752440) * a + 1.0)
    p = f(0.5 * 1.061405429) * t + f(0.5 * -1.453152027)
    p = p * t + f(0.5 * 1.421413741)
    p = p * t + f(0.5 * -0.284496736)
    p = p * t + f(0.5 * 0.254829592)
    q = p * t * torch.exp2(f(-0.5 * 1.4426950408889634) * x * x)
    phi = 0.5 + torch.copysign(0.5 - q, x)
    return x * phi


def gelu_tanh_fp32(x):
    return F.gelu(x.float(), approximate="tanh")


def quick_gelu_17_fp32(x):
    return x.float() * torch.sigmoid(1.7 * x.float())


def swiglu_fp32(gu, mutant=None):
    Fh = gu.shape[-1] // 2
    g, u = gu[..., :Fh].float(), gu[..., Fh:].float()
    if mutant == "SwiGLU with gate and up swapped":
        g, u = u, g
    s = F.silu(g)
    if gu.dtype == BF and mutant != "SwiGLU without the bf16 rounding of the gate":
        s = s.to(BF).float()
    return s * u


def rope_axial_fp32(x, cos, sin, n_rope, n_grid, mutant=None):
    """a c - b s, a s + b c in fp32 on the first n_rope tokens -> fp32 [B, n_rope, C]; the mutant reads the table row of tok, not tok % n_grid"""
    B, N, C = x.shape
    xr = x[:, :n_rope].float().reshape(B, n_rope, C // 2, 2)
    idx = torch.arange(n_rope) if mutant else torch.arange(n_rope) % n_grid
    c, s = cos[idx][None], sin[idx][None]
    a, b = xr[..., 0], xr[..., 1]
    return torch.stack([a * c - b * s, a * s + b * c], dim=-1).reshape(B, n_rope, C)
