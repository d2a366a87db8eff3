"""The fp8 K/V cache of the decode step (cfg["llm"]["kv_cache"] = "fp8") on the host: the config key's default and validation, every
refusal, which B-row step goes with the mode at each width, and the format's torch statement on the ties and the saturation edges."""
import pytest
import torch

import _golden as G

torch.set_grad_enabled(False)

BF16, F32 = torch.bfloat16, torch.float32


def _mode(value, dtype=BF16, device="cuda", fused=True, env=None):
    from videoglamm_amd.vlm import kv_cache_mode
    return kv_cache_mode(value, dtype, device, fused, env or {})


def test_default_is_bf16():
    assert _mode(None) is False and _mode("bf16") is False
    # the default takes no look at the rest: an fp32 CPU model without the fused kernels under the chained launch keeps its cache
    assert _mode(None, F32, "cpu", False, {"VG_DECODE_CHAIN": "3"}) is False
    assert _mode("bf16", F32, "cpu", False, {"VG_DECODE_CHAIN": "3"}) is False
    assert _mode("fp8") is True
    assert _mode("fp8", env={"VG_DECODE_CHAIN": "0"}) is True


@pytest.mark.parametrize("value", ["e4m3", "fp16", "FP8", 8, True, ""])
def test_unknown_value_is_refused(value):
    with pytest.raises(ValueError, match="kv_cache"):
        _mode(value)


@pytest.mark.parametrize("kw,word", [(dict(dtype=F32), "bf16 model"), (dict(device="cpu"), "GPU"), (dict(fused=False), "fused decode kernels"),
                                     (dict(env={"VG_DECODE_CHAIN": "1"}), "VG_DECODE_CHAIN"), (dict(env={"VG_DECODE_CHAIN": "3"}), "VG_DECODE_CHAIN")])
def test_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        _mode("fp8", **kw)


def test_step_form_and_route():
    """Phi-3-mini width keeps its B-row step (and so batches); Llama-3 width loses the rope step and has no B-row step (and so loops)"""
    from videoglamm_amd import prompts
    from videoglamm_amd.vlm import decode_step_form
    # (rope covered, decode_attention rows covered): Llama-3 width = (True, False), Phi-3-mini width = (False, True), neither = (False, False)
    assert decode_step_form(True, False) == "rope" and decode_step_form(False, True) == "attention" and decode_step_form(False, False) is None
    assert decode_step_form(True, True) == "rope"
    assert decode_step_form(False, True, kv8=True) == "attention"
    assert decode_step_form(True, False, kv8=True) is None
    assert decode_step_form(True, True, kv8=True) == "attention"
    r = ["greedy"] * 4
    for switch in ("VG_PROMPTS_BATCHED", "VG_CLIPS_BATCHED"):
        for width, (rope, attn) in dict(phi3=(False, True), llama=(True, False)).items():
            step = decode_step_form(rope, attn, kv8=True)
            got = prompts.batched_route(4, step == "rope", None, 0, r, {}, attn_rows=step == "attention", switch=switch)
            assert got == (width == "phi3"), (switch, width)
            assert not prompts.batched_route(4, step == "rope", None, 0, r, {switch: "0"}, attn_rows=step == "attention", switch=switch)


@pytest.mark.parametrize("gemv", ["mfma", "mfma_q"])
def test_decode_gemv_without_its_step_is_refused(gemv):
    from videoglamm_amd.vlm import decode_step_form, kv_cache_check_gemv
    with pytest.raises(ValueError, match="decode_gemv"):
        kv_cache_check_gemv(gemv, decode_step_form(True, False, kv8=True))       # Llama-3 width: the rope step is gone
    kv_cache_check_gemv(gemv, decode_step_form(False, True, kv8=True))           # Phi-3-mini width keeps the rows step
    kv_cache_check_gemv(None, None)
    kv_cache_check_gemv("valu", None)


def _tiny(dtype):
    from videoglamm_amd.params import Params
    c = G.configs.PHI3_TINY
    sd = {"model." + k: v for k, v in G.weights("phi3_tiny_manifest.json", 5).items()}
    return Params(sd, torch.device("cpu"), dtype), c


@pytest.mark.parametrize("dtype,word", [(F32, "bf16 model"), (BF16, "GPU")])
def test_decoder_refuses_before_any_work(dtype, word):
    from videoglamm_amd.vlm import LlamaDecoder
    P, c = _tiny(dtype)
    with pytest.raises(ValueError, match=word):
        LlamaDecoder(P, dict(c, kv_cache="fp8"), 64)
    with pytest.raises(ValueError, match="kv_cache"):
        LlamaDecoder(P, dict(c, kv_cache="int8"), 64)
    dec = LlamaDecoder(P, c, 64)
    assert dec.kv8 is False and dec.kc8 is None and dec.vc8 is None
    assert LlamaDecoder(P, dict(c, kv_cache="bf16"), 64).kv8 is False


def test_forward_sharded_is_refused():
    """a multi-GPU model's sequence-parallel prefill: refused before it touches the comm or the caches"""
    from videoglamm_amd.vlm import LlamaDecoder
    P, c = _tiny(F32)
    dec = LlamaDecoder(P, c, 64)
    dec.kv8 = True              # (no CPU decoder takes the mode: the refusal itself is what runs here)
    with pytest.raises(ValueError, match="forward_sharded"):
        dec.forward_sharded(torch.zeros(8, c["hidden"]), None)


# ------------------------------------------------------------------ the format: x.float().clamp(-448, 448).to(torch.float8_e4m3fn)
def _codes(vals):
    from videoglamm_amd import ops
    return ops.kv_quantize_reference(torch.tensor(vals, dtype=torch.float32).to(BF16)).tolist()


def test_reference_statement_on_ties_and_saturation():
    from videoglamm_amd import ops
    assert _codes([0.0, -0.0, 1.0, -1.0, 448.0, -448.0]) == [0x00, 0x80, 0x38, 0xB8, 0x7E, 0xFE]
    assert _codes([449.0, -449.0, 1e4, -1e4, float("inf"), float("-inf")]) == [0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0xFE]       # saturation, never NaN
    assert _codes([2.0 ** -9, 2.0 ** -10, 2.0 ** -11, -2.0 ** -10, 3 * 2.0 ** -10]) == [0x01, 0x00, 0x00, 0x80, 0x02]     # flush; ties to even
    assert _codes([432.0, 400.0, 1.0625, 1.1875]) == [0x7E, 0x7C, 0x38, 0x3A]                                             # ties to even
    assert _codes([float("nan")])[0] & 0x7F == 0x7F       # a NaN stays a NaN code (the sign of a NaN is the clamp's to choose)
    # every finite code survives the round trip, and its bf16 value is exact
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    deq = ops.kv_dequantize(codes)
    assert deq.dtype == BF16 and torch.equal(deq.float(), codes.view(torch.float8_e4m3fn).float())
    assert torch.equal(ops.kv_quantize_reference(deq), codes)
    # the midpoint of two neighbours goes to the one with the even code
    pos = torch.arange(0, 0x7F, dtype=torch.uint8)
    v = pos.view(torch.float8_e4m3fn).float()
    mid = ((v[:-1] + v[1:]) / 2).to(BF16)
    assert torch.equal(mid.float(), (v[:-1] + v[1:]) / 2)                    # the midpoints are bf16 values
    want = torch.where(pos[:-1] % 2 == 0, pos[:-1], pos[1:])
    assert torch.equal(ops.kv_quantize_reference(mid), want)
    assert torch.equal(ops.kv_quantize_reference(-mid), want | 0x80)
