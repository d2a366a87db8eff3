"""The decode mode cfg["llm"]["decode_gemv"] = "mfma"  on the host: the kernel is exported and bound, the mode's acceptance and refusal
rules as the pure function vlm.decode_gemv_mode, and prompts.batched_route — which the mode does not touch — on every combination the batched
multi-prompt tests enumerate."""
import inspect

import pytest
import torch

LLAMA = [(4096, 4096), (14336, 4096), (4096, 14336), (128256, 4096)]                  # o, gate|up (per half), down, lm_head
PHI3 = [(3072, 3072), (8192, 3072), (3072, 8192), (32064, 3072), (9216, 3072)]        # ... and q|k|v


def test_kernel_is_exported_and_bound():
    import __graft_entry__ as g

    g.build()
    from videoglamm_amd import _lib, ops

    lib = _lib.load()
    assert hasattr(lib, "vg_decode_gemm_rows") and hasattr(lib, "vg_decode_gemm_rows_supported")
    assert {"vg_decode_gemm_rows", "vg_decode_gemm_rows_supported"} <= set(_lib.EXPORTS)
    assert callable(ops.decode_gemm_rows)
    for K in (3072, 4096, 8192, 14336):
        assert ops.decode_gemm_rows_supported(16, K) and ops.decode_gemm_rows_supported(128256, K)
        assert ops.decode_gemm_rows_supported(128257, K) and ops.decode_gemm_rows_supported(32012, K)      # vocabularies with added tokens: a ragged last tile
        assert not ops.decode_gemm_rows_supported(0, K) and not ops.decode_gemm_rows_supported(-16, K)
    for K in (2048, 3080, 6144, 16384, 0):
        assert not ops.decode_gemm_rows_supported(4096, K)
    assert all(ops.decode_gemm_rows_supported(N, K) for N, K in LLAMA + PHI3)


def _mode(value="mfma", decode_weights=None, dtype=torch.bfloat16, env=None, step="rope", projections=None, supported=None):
    from videoglamm_amd import vlm

    sup = supported or (lambda N, K: N > 0 and K in (3072, 4096, 8192, 14336))
    return vlm.decode_gemv_mode(value, decode_weights, dtype, env or {}, step, LLAMA if projections is None else projections, sup)


def test_mode_default_is_absent():
    assert _mode(value=None) is False and _mode(value="valu") is False
    # the default asks nothing of the decoder: every combination the mode refuses stays what it was
    assert _mode(value=None, decode_weights="fp8", dtype=torch.float32, env={"VG_DECODE_CHAIN": "3", "VG_DECODE_AHEAD": "1"}, step=None,
                 projections=[(33, 100)]) is False


def test_mode_accepted():
    assert _mode() is True                                              # Llama-3 width, the rope step
    assert _mode(step="attention", projections=PHI3) is True            # Phi-3-mini width, the decode_attention rows step
    assert _mode(decode_weights="bf16") is True
    assert _mode(env={"VG_DECODE_CHAIN": "0", "VG_DECODE_AHEAD": "0", "VG_PROMPTS_BATCHED": "0", "VG_CLIPS_BATCHED": "0"}) is True


@pytest.mark.parametrize("kw,word", [
    (dict(decode_weights="fp8"), "fp8"),
    (dict(decode_weights="mxfp4"), "mxfp4"),
    (dict(dtype=torch.float32), "bf16"),
    (dict(env={"VG_DECODE_CHAIN": "1"}), "VG_DECODE_CHAIN"),
    (dict(env={"VG_DECODE_CHAIN": "3"}), "VG_DECODE_CHAIN"),
    (dict(env={"VG_DECODE_AHEAD": "1"}), "VG_DECODE_AHEAD"),
    (dict(value="wmma"), "wmma"),
    (dict(value=True), "True"),
    (dict(step=None), "step"),
    (dict(projections=[(4096, 4096), (11008, 4096), (4096, 11008)]), "11008"),      # a K the kernel does not walk
    (dict(projections=[(4096, 4096), (32001, 5120)]), "5120"),
])
def test_mode_refused_with_the_reason(kw, word):
    with pytest.raises(ValueError) as e:
        _mode(**kw)
    assert word in str(e.value)


def test_mode_asks_the_kernel_about_every_projection():
    seen = []
    assert _mode(supported=lambda N, K: seen.append((N, K)) or True)
    assert seen == LLAMA


# ---- prompts.batched_route: the mode only changes which GEMV the step calls
ROUTE_CASES = [        # (kwargs over the defaults below, result) — the combinations of tests/test_prompts_batched*.py
    (dict(), True), (dict(B=2, routes=["sample_fast"] * 2), True), (dict(B=16, routes=["sample"] * 16), True),
    (dict(B=1, routes=["greedy"]), False), (dict(B=17, routes=["greedy"] * 17), False), (dict(rope_path=False), False),
    (dict(decode_weights="fp8"), False), (dict(chain=1), False), (dict(routes=["greedy", "sample_fast", "greedy", "greedy"]), False),
    (dict(routes=["sample", "sample_fast", "sample", "sample"]), False), (dict(env={"VG_PROMPTS_BATCHED": "0"}), False),
    (dict(env={"VG_DECODE_AHEAD": "1"}), False),
    (dict(rope_path=False, attn_rows=True), True), (dict(rope_path=False, attn_rows=False), False),
    (dict(decode_weights="fp8", w8_rows=True), True), (dict(decode_weights="fp8", w8_rows=True, rope_path=False, attn_rows=True), True),
    (dict(decode_weights="fp8", w8_rows=False, rope_path=False, attn_rows=True), False), (dict(decode_weights="fp8", w8_rows=True, chain=1), False),
    (dict(decode_weights="fp8", w8_rows=True, env={"VG_DECODE_AHEAD": "1"}), False), (dict(decode_weights="bf16", w8_rows=True), True),
    (dict(decode_weights=None, rope_path=False, attn_rows=False, w8_rows=True), False),
    (dict(decode_weights="mxfp4"), False), (dict(decode_weights="mxfp4", w4_rows=True), True), (dict(decode_weights="mxfp4", w8_rows=True), False),
    (dict(decode_weights="mxfp4", w4_rows=True, rope_path=False, attn_rows=True), True), (dict(decode_weights="mxfp4", w4_rows=True, chain=1), False),
    (dict(decode_weights=None, w4_rows=True, rope_path=False), False),
    (dict(switch="VG_CLIPS_BATCHED", env={"VG_PROMPTS_BATCHED": "0"}), True), (dict(switch="VG_CLIPS_BATCHED", env={"VG_CLIPS_BATCHED": "0"}), False),
]


@pytest.mark.parametrize("kw,want", ROUTE_CASES)
def test_batched_route_is_unchanged(kw, want):
    from videoglamm_amd import prompts

    a = dict(B=4, rope_path=True, decode_weights=None, chain=0, routes=["greedy"] * 4, env={}, attn_rows=False, w8_rows=False, w4_rows=False,
             switch="VG_PROMPTS_BATCHED")
    a.update(kw)
    got = prompts.batched_route(a["B"], a["rope_path"], a["decode_weights"], a["chain"], a["routes"], a["env"], attn_rows=a["attn_rows"],
                                w8_rows=a["w8_rows"], w4_rows=a["w4_rows"], switch=a["switch"])
    assert bool(got) is want


def test_batched_route_takes_no_new_argument():
    from videoglamm_amd import prompts

    assert list(inspect.signature(prompts.batched_route).parameters) == ["B", "rope_path", "decode_weights", "chain", "routes", "env", "attn_rows",
                                                                         "w8_rows", "w4_rows", "switch"]
