"""The fp8 K/V cache on the rope decode step (cfg["llm"]["kv_cache"] = "fp8_rope") on the host: the new config value, every refusal by
message word, which step form and which batched route go with the mode, and the ops / library tables the mode needs."""
import pytest
import torch

import _golden as G

torch.set_grad_enabled(False)

BF16, F32 = torch.bfloat16, torch.float32


def _mode(value, dtype=BF16, device="cuda", fused=True, env=None):
    from videoglamm_amd.vlm import kv_cache_mode
    return kv_cache_mode(value, dtype, device, fused, env or {})


def test_value_is_accepted_and_distinct():
    got = _mode("fp8_rope")
    assert got and got is not True and got == "rope"
    assert _mode("fp8_rope", env={"VG_DECODE_CHAIN": "0"}) == "rope"
    assert _mode("fp8") is True and _mode(None) is False and _mode("bf16") is False      # the other values keep their answers


@pytest.mark.parametrize("value", ["fp8-rope", "rope", "FP8_ROPE", "fp8_rope ", ("fp8_rope",)])
def test_near_misses_are_refused(value):
    with pytest.raises(ValueError, match="fp8_rope"):           # the message lists the values there are
        _mode(value)


@pytest.mark.parametrize("kw,word", [(dict(dtype=F32), "bf16 model"), (dict(device="cpu"), "GPU"), (dict(fused=False), "fused decode kernels"),
                                     (dict(env={"VG_DECODE_CHAIN": "1"}), "VG_DECODE_CHAIN"), (dict(env={"VG_DECODE_CHAIN": "3"}), "VG_DECODE_CHAIN")])
def test_refusals_are_fp8s(kw, word):
    with pytest.raises(ValueError, match=word) as e:
        _mode("fp8_rope", **kw)
    assert "'fp8_rope'" in str(e.value)                         # and they name the value that was asked for


def test_step_form():
    from videoglamm_amd.vlm import decode_step_form, kv_cache_check_gemv, kv_cache_check_rope
    rope = _mode("fp8_rope")
    # (rope covered, decode_attention rows covered): Llama-3 width = (True, False), Phi-3-mini width = (False, True)
    assert decode_step_form(True, False, kv8=rope) == "rope" and decode_step_form(True, True, kv8=rope) == "rope"
    assert decode_step_form(False, True, kv8=rope) is None and decode_step_form(False, False, kv8=rope) is None
    # two positional arguments, and kv8=True / False, answer as before
    assert decode_step_form(True, False) == "rope" and decode_step_form(False, True) == "attention" and decode_step_form(False, False) is None
    assert decode_step_form(True, False, kv8=True) is None and decode_step_form(True, True, kv8=True) == "attention"
    assert decode_step_form(True, False, kv8=False) == "rope" and decode_step_form(True, False, False) == "rope"
    kv_cache_check_rope("rope")
    for step in (None, "attention"):
        with pytest.raises(ValueError, match="rope step") as e:
            kv_cache_check_rope(step)
        assert "kv_cache = 'fp8'" in str(e.value) and "VG_DECODE_ROPE" in str(e.value) and "Phi-3-mini" in str(e.value)
    for gemv in (None, "valu", "mfma", "mfma_q"):              # the MFMA projections keep their step in the mode
        kv_cache_check_gemv(gemv, decode_step_form(True, False, kv8=rope))


def test_batched_route():
    from videoglamm_amd import prompts
    from videoglamm_amd.vlm import decode_step_form
    r = ["greedy"] * 4
    step = decode_step_form(True, False, kv8=_mode("fp8_rope"))
    for switch in ("VG_PROMPTS_BATCHED", "VG_CLIPS_BATCHED"):
        assert prompts.batched_route(4, step == "rope", None, 0, r, {}, attn_rows=step == "attention", switch=switch)
        assert prompts.batched_route(4, step == "rope", None, 0, r, {switch: "1"}, attn_rows=step == "attention", switch=switch)
        assert not prompts.batched_route(4, step == "rope", None, 0, r, {switch: "0"}, attn_rows=step == "attention", switch=switch)
    # the slots of the mode start at a multiple of the rope form's keys per workgroup, as the bf16 slots do
    assert prompts.slot_layout(835, 256, 900)[0] == 768 and prompts.slot_layout(835, 128, 900)[0] == 768 and prompts.slot_layout(100, 256, 300)[0] == 0


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
        LlamaDecoder(P, dict(c, kv_cache="fp8_rope"), 64)


def test_forward_sharded_is_refused():
    from videoglamm_amd.vlm import LlamaDecoder
    P, c = _tiny(F32)
    dec = LlamaDecoder(P, c, 64)
    dec.kv8 = "rope"            # (no CPU decoder takes the mode: the refusal itself is what runs here)
    with pytest.raises(ValueError, match="forward_sharded"):
        dec.forward_sharded(torch.zeros(8, c["hidden"]), None)


def test_ops_and_exports():
    from videoglamm_amd import _lib, ops
    for name in ("decode_qkv_rope_kv8", "decode_attention2_kv8", "decode_qkv_rope_rows_kv8", "decode_attention2_rows_kv8", "decode_rope_path_kv8"):
        assert callable(getattr(ops, name)), name
    # each byte-cache entry point is exported and takes its bf16 twin's arguments
    lib = _lib.load()
    for name in ("vg_decode_qkv_rope", "vg_decode_attention2", "vg_decode_qkv_rope_rows", "vg_decode_attention2_rows", "vg_decode_attention2_supported"):
        stem, tail = (name[:-len("_supported")], "_supported") if name.endswith("_supported") else (name, "")
        twin = stem + "_kv8" + tail
        assert twin in _lib.EXPORTS, twin
        assert getattr(lib, twin).argtypes == getattr(lib, name).argtypes and getattr(lib, twin).restype == getattr(lib, name).restype, twin
    # the shapes are the rope path's, in bf16 only (no device work: the answers come from the library's host code)
    assert ops.decode_rope_path_kv8(32, 8, 128, 4096, BF16) and ops.decode_rope_path_kv8(16, 8, 128, 2048, BF16)
    assert not ops.decode_rope_path_kv8(32, 8, 128, 4096, F32) and not ops.decode_rope_path_kv8(32, 32, 96, 3072, BF16)
    assert not ops.decode_rope_path_kv8(32, 8, 128, 8192, BF16)
