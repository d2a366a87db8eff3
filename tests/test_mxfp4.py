"""MXFP4 decode weights (cfg["llm"]["decode_weights"] = "mxfp4") on the host: the quantiser against an independent statement of the OCP
Microscaling v1.0 rule, the error bound that follows from the format, the packed-row layout round trip, and the batched route's refusal."""
import itertools
import math

import numpy as np
import pytest
import torch

from videoglamm_amd import ops, prompts

KS = (3072, 4096, 8192, 14336)
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # e2m1 magnitudes by code


def spec_block(block):
    """32 values -> (32 codes, scale byte) from the text of the spec, in float64 and plain Python: shared exponent floor(log2 amax) - emax_elem
    (e2m1: emax 2), elements to the nearest grid value, a tie to the even code, magnitudes beyond 6 saturate, the sign kept (of a zero too)."""
    v = np.asarray(block, dtype=np.float64)
    amax = np.abs(v).max()
    if amax == 0:
        e = -127
    else:
        m, ex = math.frexp(float(amax))              # amax = m * 2^ex, 0.5 <= m < 1
        e = min(max(ex - 1 - 2, -127), 127)
    codes = []
    for x in v:
        a = abs(float(x)) / 2.0 ** e
        best = min(range(8), key=lambda c: (abs(GRID[c] - a), c % 2))     # nearest; of two equally near codes the even one
        codes.append(best | (8 if np.signbit(x) else 0))
    return codes, e + 127


def spec_rows(w):
    N, K = w.shape
    codes = np.zeros((N, K // 2), dtype=np.uint8)
    scales = np.zeros((N, K // 32), dtype=np.uint8)
    for n in range(N):
        for b in range(K // 32):
            c, s = spec_block(w[n, 32 * b:32 * b + 32].double().numpy())
            scales[n, b] = s
            for j in range(16):
                codes[n, 16 * b + j] = c[2 * j] | (c[2 * j + 1] << 4)
    return torch.from_numpy(codes), torch.from_numpy(scales)


def weights(K, seed=0, rows=3):
    """seeded N(0, K^-1) rows in bf16 with the cases the rule has to get right planted in row 0"""
    w = (torch.randn(rows, K, generator=torch.Generator().manual_seed(seed)) * K ** -0.5).to(torch.bfloat16).float()
    w[0, 0:32] = 0.0                                                  # an all-zero block
    w[0, 32:64] = torch.linspace(-0.9, 0.9, 32)
    w[0, 40] = 1.0                                                    # amax a power of two: e = -2, 1.0 is the code of 4
    w[0, 64:96] = 0.0
    w[0, 64] = 4.0                                                    # e = 0: the grid itself ...
    w[0, 65:72] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25])     # ... and values exactly on its ties
    w[0, 72:76] = torch.tensor([-0.75, -2.5, 0.5, -1.5])
    w[0, 96:128] = 0.0
    w[0, 96] = 7.5                                                    # e = 0 and 7.5 in (6, 8): saturates at 6
    w[0, 97] = -7.0
    w[0, 98] = 5.0                                                    # the tie between 4 and 6
    w[0, 128:160] = 0.01
    w[0, 130] = -0.0                                                  # a negative zero keeps its sign bit
    return w


@pytest.mark.parametrize("K", KS)
def test_quantiser_equals_the_spec(K):
    w = weights(K, seed=K)
    codes, scales = ops.quantize_mxfp4_rows(w)
    assert codes.dtype == torch.uint8 and codes.shape == (3, K // 2) and scales.dtype == torch.uint8 and scales.shape == (3, K // 32)
    want_c, want_s = spec_rows(w)
    assert torch.equal(scales, want_s)
    assert torch.equal(codes, want_c)
    # the planted cases read back: zero block, the power of two, the ties, the saturation, the negative zero
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(3, K)
    assert int(scales[0, 0]) == 0 and not nib[0, :32].any()
    assert int(scales[0, 1]) == 127 - 2 and int(nib[0, 40]) == 6
    assert int(scales[0, 2]) == 127 and nib[0, 64:76].tolist() == [6, 0, 2, 2, 4, 4, 6, 8, 8 | 2, 8 | 4, 1, 8 | 3]
    assert int(scales[0, 3]) == 127 and nib[0, 96:99].tolist() == [7, 8 | 7, 6]
    assert int(nib[0, 130]) == 8
    # bf16 weights give the same codes as their fp32 values (the decoder quantises the packed model-dtype weight)
    c16, s16 = ops.quantize_mxfp4_rows(w.to(torch.bfloat16))
    assert torch.equal(c16, codes) and torch.equal(s16, scales)


@pytest.mark.parametrize("K", KS)
def test_error_bound_of_the_format(K):
    """|dequant - w| <= amax_block / 4: the widest grid step is 2 * 2^e (4 | 6; half of it is the rounding error), saturation loses less than
    2 * 2^e, and 4 * 2^e <= amax_block"""
    w = weights(K, seed=K + 1, rows=5)
    w[1] *= 2.0 ** 40
    w[2] *= 2.0 ** -60
    codes, scales = ops.quantize_mxfp4_rows(w)
    deq = ops.mxfp4_dequant(codes, scales)
    assert deq.dtype == torch.float32 and deq.shape == w.shape
    amax = w.reshape(5, K // 32, 32).abs().amax(dim=-1, keepdim=True)
    assert bool(((deq - w).reshape(5, K // 32, 32).abs() <= 0.25 * amax).all())
    assert bool((deq[0, :32] == 0).all())


@pytest.mark.parametrize("K", KS)
def test_pack_round_trip_and_bf16_exactness(K):
    w = weights(K, seed=K + 2)
    codes, scales = ops.quantize_mxfp4_rows(w)
    packed = ops.mxfp4_pack(codes, scales)
    spl = ops.MXFP4_K[K]
    assert packed.dtype == torch.uint8 and packed.shape == (3, 64 * spl + K // 2) and packed.shape[1] % 16 == 0 and packed.is_contiguous()
    # the layout the header states: head byte lane * SPL + u = the scale of block 64 u + lane (0 where there is none), then the logical codes
    for lane, u in itertools.product((0, 1, 31, 32, 63), range(spl)):
        blk = 64 * u + lane
        assert int(packed[1, lane * spl + u]) == (int(scales[1, blk]) if blk < K // 32 else 0)
    assert torch.equal(packed[:, 64 * spl:], codes)
    deq = ops.mxfp4_dequant(codes, scales)
    assert torch.equal(ops.mxfp4_dequant(packed), deq) and torch.equal(ops.mxfp4_dequant(packed, K=K), deq)
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)             # two significant bits times a power of two: exact in bf16
    c2, s2 = ops.quantize_mxfp4_rows(deq)                               # and a fixed point of the quantiser
    assert torch.equal(ops.mxfp4_dequant(c2, s2), deq)
    if hasattr(torch, "float4_e2m1fn_x2"):                              # the logical layout is torch's: the codes view as its packed dtype
        assert codes.view(torch.float4_e2m1fn_x2).shape == codes.shape


def test_params_fp4_caches_the_packed_rows():
    from videoglamm_amd.params import Params
    g = torch.Generator().manual_seed(1)
    sd = {"a.gate_proj.weight": torch.randn(8, 4096, generator=g), "a.up_proj.weight": torch.randn(8, 4096, generator=g),
          "a.down_proj.weight": torch.randn(6, 8192, generator=g), "b.gate_up_proj.weight": torch.randn(16, 3072, generator=g)}
    P = Params(sd, "cpu", torch.bfloat16)
    gu = P.fp4(["a.gate_proj", "a.up_proj"], stored="a.gate_up_proj")
    assert gu.shape == (16, 128 + 2048) and P.fp4(["a.gate_proj", "a.up_proj"], stored="a.gate_up_proj") is gu
    want = torch.cat([sd["a.gate_proj.weight"], sd["a.up_proj.weight"]]).to(torch.bfloat16)
    assert torch.equal(gu, ops.mxfp4_pack(*ops.quantize_mxfp4_rows(want)))
    assert P.fp4("a.down_proj").shape == (6, 256 + 4096)
    st = P.fp4(["b.gate_proj", "b.up_proj"], stored="b.gate_up_proj")    # Phi-3's stored fused form
    assert torch.equal(st, ops.mxfp4_pack(*ops.quantize_mxfp4_rows(sd["b.gate_up_proj.weight"].to(torch.bfloat16))))


# ------------------------------------------------------------------ the batched route
def _parent_rule(B, rope_path, decode_weights, chain, routes, env, attn_rows=False, w8_rows=False):
    """prompts.batched_route as it stood before "mxfp4" existed"""
    return (2 <= B <= 16 and (bool(rope_path) or bool(attn_rows)) and (decode_weights != "fp8" or bool(w8_rows)) and not chain
            and len(set(routes)) == 1 and env.get("VG_PROMPTS_BATCHED", "1") != "0" and env.get("VG_DECODE_AHEAD", "0") != "1")


def test_batched_route_refuses_mxfp4_without_a_rows_kernel():
    r = ["greedy"] * 4
    assert not prompts.batched_route(4, True, "mxfp4", 0, r, {})
    assert not prompts.batched_route(4, True, "mxfp4", 0, r, {}, w8_rows=True)
    assert not prompts.batched_route(4, False, "mxfp4", 0, r, {}, attn_rows=True)
    assert prompts.batched_route(4, True, "mxfp4", 0, r, {}, w4_rows=True) is True
    assert prompts.batched_route(4, False, "mxfp4", 0, r, {}, attn_rows=True, w4_rows=True) is True
    assert not prompts.batched_route(4, False, "mxfp4", 0, r, {}, attn_rows=False, w4_rows=True)
    assert not prompts.batched_route(1, True, "mxfp4", 0, ["greedy"], {}, w4_rows=True)
    assert not prompts.batched_route(4, True, "mxfp4", 1, r, {}, w4_rows=True)
    assert not prompts.batched_route(4, True, "mxfp4", 0, r, {"VG_PROMPTS_BATCHED": "0"}, w4_rows=True)


def test_batched_route_is_unchanged_for_every_other_mode():
    """every combination the existing batched-route tests enumerate (test_prompts_batched*.py), with and without the new keyword"""
    n = 0
    for B, rope, dw, chain, mixed, env, attn, w8 in itertools.product(
            (1, 2, 4, 16, 17), (True, False), (None, "bf16", "fp8"), (0, 1), (False, True),
            ({}, {"VG_PROMPTS_BATCHED": "0"}, {"VG_DECODE_AHEAD": "1"}), (False, True), (False, True)):
        routes = ["greedy"] * B if not mixed else ["greedy", "sample_fast"] + ["greedy"] * (B - 1)
        want = _parent_rule(B, rope, dw, chain, routes, env, attn_rows=attn, w8_rows=w8)
        assert prompts.batched_route(B, rope, dw, chain, routes, env, attn_rows=attn, w8_rows=w8) == want
        for w4 in (False, True):
            assert prompts.batched_route(B, rope, dw, chain, routes, env, attn_rows=attn, w8_rows=w8, w4_rows=w4) == want
        n += 1
    assert n == 5 * 2 * 3 * 2 * 2 * 3 * 2 * 2


def test_load_in_4bit_refusal_points_at_mxfp4(monkeypatch):
    from videoglamm_amd import _lib
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    monkeypatch.setattr(_lib, "load", lambda: None)
    with pytest.raises(NotImplementedError, match=r"decode_weights'\] = 'mxfp4'"):
        VideoGLaMMForCausalLM({}, dict(seg_token_idx=1), torch_dtype=torch.bfloat16, device="cpu", load_in_4bit=True)
