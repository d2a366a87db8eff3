"""vg_twoway_image_update and vg_mask_upscale against float64 chains that round where the kernels round (-m gpu).

tests/test_kernels_gpu.py compares the two fused mask-decoder kernels with fp32 statements at rtol = atol = 3e-2 on P in {96, 256, 1024, 4096},
Nx == N and N <= 4.  At that bound eps x 10, a one-pass variance and a missing bf16 rounding of the probabilities pass the two-way test, and
eps x 1000 or a tanh GELU the upscale test (the honest chain already sits 1.4e-2 from a reference that has none of the kernel's roundings).  Here
(tests/_layout_ref.py: designs, references, wrong kernels; tests/test_layout_selfcheck.py: each wrong kernel fails on the CPU):

vg_twoway_image_update
  selector design   xpe rows two-hot, u2 / c2 in {0, -128}: every score is a multiple of 128, the live tokens of a head are those at the row maximum,
                    every other probability is exactly 0 and the live ones bf16(1 / count).  With integer w2t, bo and x, v = x + (bf16(y) + bo) is known
                    exactly (asserted on the CPU: the fp32 chain equals the float64 model); the final LayerNorm is a _rowwise_ref.norm_case on v
                    (element and share checks; every 8th row a `step` row 1024 + 8 k for the one-pass variance; eps = 0.5 so that eps x 10 shows on
                    every row), and x' + pe must equal (x'.float() + pe.float()).to(bf16) of the kernel's own x' bit for bit.  The masked columns
                    (t >= nt) of u2 / w2t hold 1000.  A wrong row, head, token, swizzle slot or instance moves v by whole integers: the lane-to-row map,
                    the permlane pairing of score columns, both swizzled LDS stagings and TP = 16's u2 straight from global memory, the slab
                    transpose, the token mask, c2 indexing, x against xpe, n % Nx.
                    Cases: TP 8 with nt in {1, 7, 8}, TP 16 with nt in {1, 8, 9, 16}, each at P = 40 (>> ragged inside the first wave), 296 (>> a second
                    workgroup, P % 32 != 0) and 1000 (>> a second `iters` pass with a break), with (N, Nx) in {(3, 3), (4, 2), (3, 1)} in rotation
                    (>> shared inputs, the kernel's nx = n % xmod: every TP meets every pair).
  random data       one case per TP against the float64 chain that rounds the probabilities and y to bf16: a tight bound (1/2 ulp_bf16 + 16 x the
                    LayerNorm unit of _rowwise_ref) that all but a share of 2e-3 of the elements must meet (the CPU fp32 statement: 5e-5 .. 2e-4) and a wide
                    one, 4 x the statement's largest error, for the elements behind a flipped bf16 tie of a probability or of y.
vg_mask_upscale     float64 chain with the kernel's two bf16 roundings (after each GELU) and fp32 output; two-level check: |err| <= 1e-4 x max(1, max |ref|)
                    for all but 1.6e-2 of the elements (the statement's own share, asserted <= 4e-3 before the kernel is looked at), 4 x the statement's
                    largest error for the rest.
  instance counts   >> N = 2, 64, 256 at es = 16: iters = 2, 4, 8, each with a second iteration (and a break from iters = 4), Bi in {1, 2} and Bi = N;
                    at N >= 64 ten instances are compared (the first, the last and those around N / 2), the output guard always.
  ragged            >> es in {5, 12, 20} (P = 25, 144, 400: the clamped rows and the r0 + l31 < P store guard).
  saturating        the index-pinning design: integer operands, every GELU argument beyond +-8.1 (asserted), so an activation is the value itself or
                    about 0: a wrong tap, channel group, pixel or image index moves an output by whole units.
  quiet             the LayerNorm2d / GELU definition case: sigma about 2^-6, arguments over [-3, 3]: eps x 10 and a tanh GELU fail.
Left out: fp32 inputs (both entry points are bf16 only and say so); P or N large enough to pass 2^31 elements (the row offsets are int64; the
model's P is 4096); the token side of the two-way block (GEMMs and attention: tests/test_contraction_exact_gpu.py, tests/test_attention_accuracy_gpu.py).

Measured on the MI355X (also DESIGN.md section 2): all cases pass, no kernel was found wrong.
  selector (21 cases)   the kernel needed at most 2.1 LayerNorm units; torch's fp32 layer_norm needs up to 63.7 on the step rows, so 11.7 - 255 are allowed;
                        mismatch share kernel 7.4e-5, statement 1.1e-4; x' + pe bit-equal everywhere; v exact on the CPU in every case.
  random (TP 8 / 16)    worst 1.56e-2 (one ulp of an output in [2, 4)) of the wide bound 0.125, as the statement; share beyond the tight bound 1.6e-4 / 4.8e-5
                        (statement 2.1e-4 / 7.6e-5) of the cap 2e-3.
  upscale (13 cases)    worst 4.7e-4 .. 1.4e-2 of 0.10 .. 0.17 (statement 2.9e-4 .. 1.4e-2); share 0 .. 1.1e-3 (statement 0 .. 1.5e-3) of 1.6e-2; the
                        saturating design: error 0 in both.  The statement of one small case (N 2, es 12) had no flipped tie on one CPU and 1.6e-4 on
                        another: hence the floor of the wide bound (one flipped tie, from the formats) in _layout_ref.upscale_check.
  The 37 tests of this file take 2 s (N = 256, Bi = 256: 0.5 s).
"""
import pytest
import torch

import _layout_ref as L
import _rowwise_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BF, F32 = L.BF, L.F32
GUARD = 256


def _api():
    from videoglamm_amd import _lib, ops
    return _lib.load(), _lib, ops


def _guarded(shape, dtype, cuda):
    n = 1
    for s in shape:
        n *= s
    big = torch.full((n + 2 * GUARD,), L.SENT, dtype=dtype, device=cuda)
    return big, big[GUARD:GUARD + n].view(shape)


def _intact(big):
    return bool((big[:GUARD] == L.SENT).all()) and bool((big[-GUARD:] == L.SENT).all())


def _twoway(d, cuda):
    """-> (x', x' + pe) on the CPU; the outputs lie in sentinel-guarded buffers (a row stored past P of the last instance would show)"""
    lib, _lib, ops = _api()
    g = {k: d[k].to(cuda) for k in ("xpe", "x", "u2", "c2", "w2t", "bo", "lw", "lb", "pe")}
    N, P = d["N"], d["P"]
    b1, xo = _guarded((N, P, 256), BF, cuda)
    b2, xpo = _guarded((N, P, 256), BF, cuda)
    p = ops._p
    rc = lib.vg_twoway_image_update(p(g["xpe"]), p(g["x"]), p(g["u2"]), p(g["c2"]), p(g["w2t"]), p(g["bo"]), p(g["lw"]), p(g["lb"]), float(d["eps"]), p(g["pe"]),
                                    p(xo), p(xpo), N, d["Nx"], P, d["nt"], d["TP"], ops._dt(g["x"]), ops._stream())
    _lib.check(rc, "vg_twoway_image_update")
    torch.cuda.synchronize()
    assert _intact(b1) and _intact(b2), "a write outside the outputs"
    return xo.cpu(), xpo.cpu()


_PAIRS = [(3, 3), (4, 2), (3, 1)]
SELECTOR = [(TP, nt, P) + _PAIRS[(i + j) % 3] for i, (TP, nt) in enumerate([(8, 1), (8, 7), (8, 8), (16, 1), (16, 8), (16, 9), (16, 16)])
            for j, P in enumerate((40, 296, 1000))]


def test_selector_cases_cover():
    for TP in (8, 16):
        assert {(N, Nx) for tp, nt, P, N, Nx in SELECTOR if tp == TP} == set(_PAIRS)


@pytest.mark.parametrize("TP,nt,P,N,Nx", SELECTOR)
def test_twoway_selector(cuda, TP, nt, P, N, Nx):
    d = L.twoway_selector(N, Nx, P, nt, TP, seed=nt + P)
    case = L.twoway_selector_case(d, f"two-way selector TP{TP} nt{nt} P{P} N{N} Nx{Nx}")
    xo, xpo = _twoway(d, cuda)
    R.check(case, xo.reshape(-1, 256))
    assert torch.equal(xpo, (xo.float() + d["pe"].float()).to(BF))


@pytest.mark.parametrize("TP,nt,P,N,Nx", [(8, 7, 296, 4, 2), (16, 9, 1000, 3, 3)])
def test_twoway_random(cuda, TP, nt, P, N, Nx):
    d = L.twoway_random(N, Nx, P, nt, TP, seed=TP)
    chk = L.twoway_random_check(d, f"two-way random TP{TP} nt{nt} P{P} N{N} Nx{Nx}")
    chk.precondition()
    xo, xpo = _twoway(d, cuda)
    chk.check(xo.reshape(-1, 256))
    assert torch.equal(xpo, (xo.float() + d["pe"].float()).to(BF))


def _upscale(d, cuda):
    lib, _lib, ops = _api()
    g = {k: d[k].to(cuda) for k in ("x", "w0", "b0", "s1", "lw", "lb", "w1", "b1", "s0", "hyper")}
    N, Bi, es = d["x"].shape[0], d["s1"].shape[0], d["es"]
    big, out = _guarded((N, 4, 4 * es, 4 * es), F32, cuda)
    out.fill_(float("nan"))          # (inside the guard: an element the kernel does not write stays NaN)
    p = ops._p
    rc = lib.vg_mask_upscale(p(g["x"]), p(g["w0"]), p(g["b0"]), p(g["s1"]), p(g["lw"]), p(g["lb"]), float(d["eps"]), p(g["w1"]), p(g["b1"]), p(g["s0"]),
                             p(g["hyper"]), p(out), N, Bi, es, ops._dt(g["x"]), ops._stream())
    _lib.check(rc, "vg_mask_upscale")
    torch.cuda.synchronize()
    assert _intact(big), "a write outside the output"
    assert bool(torch.isfinite(out).all()), "an output element was not written"
    return out.cpu()


def _instances(N):
    return None if N <= 8 else sorted({0, 1, 2, N // 2 - 1, N // 2, N // 2 + 1, N - 4, N - 3, N - 2, N - 1})


UPSCALE = [(2, 2, 16), (2, 1, 16), (64, 2, 16), (64, 64, 16), (256, 1, 16), (256, 256, 16), (3, 3, 5), (2, 1, 12), (4, 2, 20)]


@pytest.mark.parametrize("N,Bi,es", UPSCALE)
def test_mask_upscale_random(cuda, N, Bi, es):
    d = L.upscale_random(N, Bi, es, seed=N + es)
    inst = _instances(N)
    chk = L.upscale_check(d, f"mask upscale N{N} Bi{Bi} es{es} iters {8 if N >= 256 else 4 if N >= 64 else 2}", inst=inst)
    chk.precondition()
    out = _upscale(d, cuda)
    chk.check(out if inst is None else out[inst])


@pytest.mark.parametrize("design,N,Bi,es", [("saturating", 4, 2, 8), ("saturating", 6, 3, 5), ("quiet", 4, 2, 8), ("quiet", 3, 1, 12)])
def test_mask_upscale_designs(cuda, design, N, Bi, es):
    d = L.upscale_random(N, Bi, es, seed=3, design=design)
    if design == "saturating":
        a1, a2 = L.upscale_arguments(d)
        assert float(a1.abs().min()) > 8 and float(a2.abs().min()) > 8
    chk = L.upscale_check(d, f"mask upscale {design} N{N} Bi{Bi} es{es}")
    chk.precondition()
    chk.check(_upscale(d, cuda))
