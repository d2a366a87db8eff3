"""The lossless 13-bit bf16 rows of the decode step's MLP weights on the HIP kernels: ops.decode_pack13 / decode_unpack13 give back every
bit and list exactly the rows the rule calls raw; ops.decode_gemv_p13 has the bits of ops.decode_gemv on the same bf16 weights; a graph-replayed
decoder step with VG_DECODE_PACK=1 leaves the state that VG_DECODE_PACK=0 leaves.  Matrices are a few rows at the real row lengths (<= 4 MB), but for the one case that needs more than 2048 row pairs."""
import functools

import numpy as np
import pytest
import torch

torch.set_grad_enabled(False)

KS = [4096, 14336]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _gauss(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, K, generator=g) * K ** -0.5).to(torch.bfloat16)


def _pow2(e):
    """2^e as a bf16 scalar tensor (e in the normal range)"""
    return torch.tensor(2.0 ** e, dtype=torch.float64).to(torch.bfloat16)


def raw_rule(w):
    """the rule, restated in NumPy on the bf16 bits of w [N,K] (CPU): the ascending indices of the raw rows"""
    b = w.contiguous().view(torch.int16).numpy().view(np.uint16).astype(np.int64)
    E, m = (b >> 7) & 255, b & 127
    bad = ((E == 255) | ((E == 0) & (m != 0))).any(axis=1)
    nz = E > 0
    emin = np.where(nz, E, 255).min(axis=1)
    emax = np.where(nz, E, 0).max(axis=1)
    has = nz.any(axis=1)
    base = np.where(has, emin - 1, 112)                     # the smallest exponent takes code 1
    span = has & (emax - base > 30)                         # codes 1..30: at most 30 consecutive binades
    scale = has & ((base - 112 + 127 < 1) | (base - 112 + 127 > 254))       # 2^(base - 112) must be a normal fp32
    return np.nonzero(bad | span | scale)[0].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _special(K):
    """rows that exercise the rule (CPU bf16 [12, K]) and the indices of those that must be raw"""
    w = _gauss(12, K, 11 + K)
    w[1, ::7] = 0.0
    w[1, 3::11] = -0.0
    w[2] = 0.0                                              # a row of zeros
    w[2, 5] = -0.0
    w[3, 0], w[3, 1] = _pow2(-40), _pow2(-11)               # exactly 30 binades (-40 .. -11; the Gaussian entries lie inside): not raw
    w[3, 2:] = w[3, 2:].clamp(-2.0 ** -12, 2.0 ** -12)
    w[3, 2:][w[3, 2:].abs() < 2.0 ** -40] = _pow2(-20)
    w[4] = w[3]
    w[4, 1] = _pow2(-10)                                    # 31 binades: raw
    w[5, K // 2] = torch.tensor([1], dtype=torch.int16).view(torch.bfloat16)[0]       # the smallest bf16 denormal: raw
    w[6, K - 1] = float("inf")                              # raw
    w[7, 9] = float("nan")                                  # raw
    big = (w[8].double() * 2.0 ** 121)                      # every exponent at 2^114 or above: base_row > 239, the scale 2^(base_row - 112) is no fp32: raw
    w[8] = torch.where(big.abs() < 2.0 ** 114, torch.full_like(big, 2.0 ** 115), big).to(torch.bfloat16)
    w[9] = (w[9].double() * 2.0 ** -100).to(torch.bfloat16)         # small but normal, and the scale 2^(base - 112) still normal: not raw
    w[9][w[9].abs() < 2.0 ** -120] = _pow2(-110)
    return w, [4, 5, 6, 7, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_round_trip_and_raw_rows(cuda, K):
    """device unpack == the original bits; the raw list == the NumPy rule == the rows built to be raw; Gaussian rows, +-0, 30 / 31 binades,
    denormal, inf, NaN, a scale outside fp32's normal range"""
    from videoglamm_amd import ops
    w, want_raw = _special(K)
    assert raw_rule(w).tolist() == want_raw
    wd = w.to(cuda)
    packed, scale, raw = ops.decode_pack13(wd, raw_cap=False)
    assert packed.shape == (12, K // 2048 * 3328) and raw.dtype == torch.int32
    assert raw.tolist() == want_raw
    back = ops.decode_unpack13(packed, scale, raw, wd)
    assert torch.equal(_bits(back), _bits(wd))
    # the packed blocks alone carry the rows that are not raw: with another matrix as "original" only the raw rows change
    other = torch.zeros_like(wd)
    back2 = ops.decode_unpack13(packed, scale, raw, other)
    keep = [r for r in range(12) if r not in want_raw]
    assert torch.equal(_bits(back2[keep]), _bits(wd[keep])) and not bool(back2[want_raw].any())
    sc = scale.cpu()
    assert bool((sc[want_raw] == 1.0).all())
    m, e = torch.frexp(sc)
    assert bool((m == 0.5).all())                           # powers of two
    assert float(sc[2]) == 1.0                              # the row of zeros


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_gaussian_matrix_packs_under_the_cap(cuda, K):
    from videoglamm_amd import ops
    rows = 512 if K == 4096 else 146
    w = _gauss(rows, K, 5 + K)
    wd = w.to(cuda)
    got = ops.decode_pack13(wd)
    want = raw_rule(w)
    assert len(want) * 256 <= rows and got is not None      # synth-like rows: (almost) none raw
    packed, scale, raw = got
    assert np.array_equal(raw.cpu().numpy(), want)
    assert torch.equal(_bits(ops.decode_unpack13(packed, scale, raw, wd)), _bits(wd))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_matrix_over_the_raw_cap_is_unpackable(cuda, K):
    """more than 1/256 of the rows raw: decode_pack13 reports None; exactly 1/256 still packs"""
    from videoglamm_amd import ops
    w = _gauss(256, K, 6 + K)
    assert len(raw_rule(w)) == 0
    w[17, 3] = float("inf")
    assert ops.decode_pack13(w.to(cuda)) is not None        # 1 of 256
    w[200, 0] = float("inf")
    assert raw_rule(w).tolist() == [17, 200]
    assert ops.decode_pack13(w.to(cuda)) is None            # 2 of 256
    assert ops.decode_pack13(w.to(cuda), raw_cap=False)[2].tolist() == [17, 200]


# ------------------------------------------------------------------ the GEMV against decode_gemv on the same bf16 weights
def _spoil(w, rows):
    """make `rows` raw, alternating the reasons (a span of 40 binades / a bf16 denormal, which meets x = 0)"""
    for i, r in enumerate(rows):
        if i % 2 == 0:
            w[r, 1], w[r, 2] = _pow2(-45), _pow2(-5)
        else:
            w[r, 4] = torch.tensor([3], dtype=torch.int16).view(torch.bfloat16)[0]
    return w


def _x(K, norm, seed, zero_at=()):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(1, K, generator=g) * (2.0 if norm else 0.5)).to(torch.bfloat16)
    for k in zero_at:
        x[0, k] = 0.0
    nw = (1.0 + 0.1 * torch.randn(K, generator=g)) if norm else None
    return x, nw


def _pair(cuda, w, x, nw, glu, res, odt, raw_expected=None):
    """decode_gemv_p13 into a buffer with sentinels around the output, twice, and decode_gemv on the same weights: all three equal, sentinels whole"""
    from videoglamm_amd import ops
    wd, xd = w.to(cuda), x.to(cuda)
    nwd = None if nw is None else nw.to(cuda)
    N = w.shape[0] // 2 if glu else w.shape[0]
    r = None
    if res:
        r = torch.randn(1, N, generator=torch.Generator().manual_seed(N)).to(odt).to(cuda)
    packed, scale, raw = ops.decode_pack13(wd, raw_cap=False)
    if raw_expected is not None:
        assert raw.tolist() == sorted(raw_expected)
    want = ops.decode_gemv(xd, wd, norm_w=nwd, eps=1e-5, residual=r, glu=glu, out_dtype=odt)
    pad = 64
    buf = torch.full((N + 2 * pad,), -3.0, dtype=odt, device=cuda)
    out = buf[pad:pad + N].view(1, N)
    got = ops.decode_gemv_p13(xd, wd, packed, scale, raw, norm_w=nwd, eps=1e-5, residual=r, glu=glu, out_dtype=odt, out=out)
    first = got.clone()
    assert bool((buf[:pad] == -3.0).all()) and bool((buf[pad + N:] == -3.0).all())
    got2 = ops.decode_gemv_p13(xd, wd, packed, scale, raw, norm_w=nwd, eps=1e-5, residual=r, glu=glu, out_dtype=odt, out=out)
    ib = torch.int16 if odt == torch.bfloat16 else torch.int32
    assert torch.equal(first.view(ib), want.view(ib))
    assert torch.equal(got2.view(ib), want.view(ib))
    return want


# the split of the launch (launch_decode_gemv): pairs per wave ppw = ceil(npair / 2048) (a wave owns ppw consecutive pairs, a workgroup 4 ppw).
#   plain N = 13 -> 7 pairs, ppw 1: the last pair is the clamped one (row 13 does not exist), waves 7.. of the second workgroup own none
#   plain N = 10 -> 5 pairs: workgroup 1 holds pair 4 in wave 0 and nothing in waves 1..3
#   GLU N = 6    -> 6 pairs: workgroup 1 holds pairs 4, 5, waves 2, 3 none
#   more than 2048 pairs (ppw 2): test_gemv_p13_bitwise_two_pairs_per_wave
CASES = [
    # name,                K,     N,    glu,   norm,  res,   fp32,  raw rows (of the stacked [2N or N, K] matrix)
    ("glu_norm",           4096,  70,   True,  True,  False, False, []),
    ("glu_plain",          4096,  70,   True,  False, False, False, [5]),
    ("glu_up_half_raw",    4096,  70,   True,  True,  False, False, [70 + 33]),
    ("glu_K14336",         14336, 66,   True,  False, True,  False, [0, 66 + 65]),
    ("plain_res",          4096,  140,  False, False, True,  False, []),
    ("plain_res_K14336",   14336, 140,  False, False, True,  False, [3, 64, 139]),
    ("plain_norm_K14336",  14336, 96,   False, True,  False, True,  [17]),
    ("odd_N",              4096,  13,   False, False, True,  False, [12]),
    ("odd_N_K14336",       14336, 13,   False, False, False, True,  [0, 11, 12]),
    ("wave_without_pairs", 4096,  10,   False, False, False, False, [8, 9]),
    ("glu_six_pairs",      14336, 6,    True,  True,  False, False, [5, 6]),
    ("several_raw",        4096,  256,  False, False, True,  False, [0, 1, 2, 7, 8, 127, 254, 255]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemv_p13_bitwise(cuda, case):
    _, K, N, glu, norm, res, f32, raw_rows = case
    w = _spoil(_gauss(2 * N if glu else N, K, N + K), raw_rows)
    x, nw = _x(K, norm, 3 * N + 1, zero_at=(4,))
    assert raw_rule(w).tolist() == sorted(raw_rows)
    want = _pair(cuda, w, x, nw, glu, res, torch.float32 if f32 else torch.bfloat16, raw_expected=raw_rows)
    assert bool(torch.isfinite(want.float()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("glu,N", [(True, 2052), (True, 2053), (False, 4104), (False, 4106), (False, 4105)])
def test_gemv_p13_bitwise_two_pairs_per_wave(cuda, glu, N):
    """a wave owns more than one pair only past 2048 pairs, so this one matrix is 34 MB (K = 4096).  2052 pairs: ppw = 2, the last workgroup's
    waves 0, 1 full, waves 2, 3 without pairs; 2053 pairs: wave 2 a partial range (one pair of its two); N = 4105: that pair is the clamped one.
    Raw rows in the first and in the last pair of a wave (pairs 2 w and 2 w + 1) and in the partial wave."""
    K = 4096
    npair = N if glu else (N + 1) // 2
    pairs = [0, 1, 2 * 700, 2 * 700 + 1, 2050, 2051, npair - 1]
    raw_rows = sorted({(p if i % 2 == 0 else N + p) if glu else min(2 * p + i % 2, N - 1) for i, p in enumerate(pairs)})
    w = _spoil(_gauss(2 * N if glu else N, K, N), raw_rows)
    x, nw = _x(K, glu, N, zero_at=(4,))
    rule = raw_rule(w).tolist()                             # (a Gaussian row of so many may be raw by itself)
    assert set(raw_rows) <= set(rule) and len(rule) <= len(raw_rows) + 2
    _pair(cuda, w, x, nw, glu, not glu, torch.bfloat16, raw_expected=rule)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shift", [20, -20])
def test_gemv_p13_bitwise_on_scaled_weights(cuda, K, shift):
    """weights times 2^+-20 (another base_row, another scale) still give the bf16 kernel's bits on those weights"""
    w = (_gauss(64, K, K + shift).double() * 2.0 ** shift).to(torch.bfloat16)
    x, nw = _x(K, False, 77)
    _pair(cuda, w, x, None, False, False, torch.float32, raw_expected=[])
    _pair(cuda, w[:64], x, None, True, False, torch.float32, raw_expected=[])


# ------------------------------------------------------------------ the decoder step
@pytest.mark.gpu
def test_step_with_packed_weights_equals_the_bf16_step(cuda, monkeypatch):
    """2-layer Llama-3-8B-width decoder, graph-replayed steps from the same prefill: VG_DECODE_PACK=1 leaves the hidden rows, the KV rows and the
    ids of VG_DECODE_PACK=0"""
    import test_prompts_batched_gpu as llama
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = llama._llm(cuda)
    c = cfg["llm"]
    S, steps = 37, 6
    x = (torch.randn(S, c["hidden"], generator=torch.Generator().manual_seed(8)) * 0.5).to(torch.bfloat16).to(cuda)

    def run(knob):
        monkeypatch.setenv("VG_DECODE_PACK", knob)
        dec = LlamaDecoder(P, c, 1024)
        assert dec.use_graph and dec.rope_path
        assert dec.proj.pack == ({"gate_up", "down"} if knob == "1" else set())
        assert dec.proj.entry("gate_up") == dec.proj.entry("down") == "decode_gemv" and dec.proj.entry("gate_up", rows=True) == "decode_gemv_rows"
        used = []
        with pytest.MonkeyPatch.context() as mp:          # count the launches that stream the 13-bit rows (made while the step is captured)
            mp.setattr(ops, "decode_gemv_p13", lambda *a, _fn=ops.decode_gemv_p13, **k: (used.append(1), _fn(*a, **k))[1])
            return steps_of(dec) + (len(used),)

    def steps_of(dec):
        h = dec.forward(x)
        dec.next_token(h[-1:])
        dec.step_dev.zero_()
        dec.advance(0)
        ids = []
        for _ in range(steps):
            ids.append(int(dec.tok_dev[0]))
            dec.decode_step()
        ids.append(int(dec.tok_dev[0]))
        n = S + steps
        return ids, dec.hid_all[:n].clone(), [k[:n].clone() for k in dec.kc], [v[:n].clone() for v in dec.vc], dec.hist[:steps + 1].tolist()

    a, b = run("0"), run("1")
    l = "model.layers.1."
    assert P.p13([l + "mlp.gate_proj", l + "mlp.up_proj"], stored=l + "mlp.gate_up_proj") is not None and P.p13(l + "mlp.down_proj") is not None
    assert a[0] == b[0] and a[4] == b[4]
    assert a[5] == 0 and b[5] == 2 * 2 * 2            # gate|up and down of two layers, in the eager step and in the captured one
    assert torch.equal(_bits(a[1]), _bits(b[1]))
    for ka, kb in zip(a[2] + a[3], b[2] + b[3]):
        assert torch.equal(_bits(ka), _bits(kb))
