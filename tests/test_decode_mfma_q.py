"""The decode mode cfg["llm"]["decode_gemv"] = "mfma_q"  on the host: the two kernels (vg_decode_gemm_w8_rows /
vg_decode_gemm_w4_rows) are exported and bound, their support queries, and the mode's acceptance and refusal rules as the pure function
vlm.decode_gemv_mode — "mfma" keeps refusing fp8 / mxfp4 decode weights."""
import inspect

import pytest
import torch

from test_decode_mfma import LLAMA, PHI3

KS = (3072, 4096, 8192, 14336)
# (N, K, kind, norm) of the quantised projections: gate|up (per half, behind the norm), down, the lm_head (always fp8)
Q_LLAMA = {dw: [(14336, 4096, k, True), (4096, 14336, k, False), (128256, 4096, "w8", False)] for dw, k in (("fp8", "w8"), ("mxfp4", "w4"))}
Q_PHI3 = {dw: [(8192, 3072, k, True), (3072, 8192, k, False), (32064, 3072, "w8", False)] for dw, k in (("fp8", "w8"), ("mxfp4", "w4"))}
BF_LLAMA = [(4096, 4096)]                          # o
BF_PHI3 = [(3072, 3072), (9216, 3072)]             # o, q|k|v


def test_kernels_are_exported_and_bound():
    import __graft_entry__ as g

    g.build()
    from videoglamm_amd import _lib, ops

    lib = _lib.load()
    names = {"vg_decode_gemm_w8_rows", "vg_decode_gemm_w8_rows_supported", "vg_decode_gemm_w4_rows", "vg_decode_gemm_w4_rows_supported"}
    assert all(hasattr(lib, n) for n in names) and names <= set(_lib.EXPORTS)
    assert callable(ops.decode_gemm_w8_rows) and callable(ops.decode_gemm_w4_rows)
    for sup in (ops.decode_gemm_w8_rows_supported, ops.decode_gemm_w4_rows_supported):
        for K in KS:
            assert sup(16, K) is True and sup(128256, K) and sup(128257, K) and sup(32012, K) and sup(33, K)      # any N > 0: a ragged last tile
            assert sup(0, K) is False and not sup(-16, K)
        for K in (2048, 3080, 6144, 16384, 0):
            assert sup(4096, K) is False
        assert all(sup(N, K) for N, K in LLAMA + PHI3)


def _sup(N, K):
    return N > 0 and K in KS


def _mode(value="mfma_q", decode_weights="fp8", dtype=torch.bfloat16, env=None, step="rope", projections=None, supported=None, quant=None,
          quant_supported=None):
    from videoglamm_amd import vlm

    q = Q_LLAMA.get(decode_weights, Q_LLAMA["fp8"]) if quant is None else quant
    return vlm.decode_gemv_mode(value, decode_weights, dtype, env or {}, step, BF_LLAMA if projections is None else projections, supported or _sup,
                                quant_projections=q, quant_supported=quant_supported or {"w8": _sup, "w4": _sup})


def test_signature_keeps_its_positional_arguments():
    from videoglamm_amd import vlm

    assert list(inspect.signature(vlm.decode_gemv_mode).parameters)[:7] == ["value", "decode_weights", "dtype", "env", "step", "projections", "supported"]


@pytest.mark.parametrize("dw", ["fp8", "mxfp4"])
def test_mode_accepted(dw):
    assert _mode(decode_weights=dw) == "mfma_q"                                                               # Llama-3 width, the rope step
    assert _mode(decode_weights=dw, step="attention", projections=BF_PHI3, quant=Q_PHI3[dw]) == "mfma_q"      # Phi-3-mini width
    assert _mode(decode_weights=dw, env={"VG_DECODE_CHAIN": "0", "VG_DECODE_AHEAD": "0", "VG_PROMPTS_BATCHED": "0", "VG_CLIPS_BATCHED": "0"}) == "mfma_q"
    assert _mode(decode_weights=dw) is not True          # dec.mfma (the bf16 mode) stays the bool it is: "mfma_q" is told apart from it


def test_other_values_keep_their_results():
    from videoglamm_amd import vlm

    a = (torch.bfloat16, {}, "rope", LLAMA, _sup)
    assert vlm.decode_gemv_mode(None, None, *a) is False and vlm.decode_gemv_mode("valu", "fp8", *a) is False
    assert vlm.decode_gemv_mode("mfma", None, *a) is True and vlm.decode_gemv_mode("mfma", "bf16", *a) is True
    for dw in ("fp8", "mxfp4"):                          # "mfma" does not silently change meaning
        with pytest.raises(ValueError, match=dw):
            vlm.decode_gemv_mode("mfma", dw, *a)
    for v in ("wmma", True):
        with pytest.raises(ValueError, match=str(v)):
            vlm.decode_gemv_mode(v, "fp8", *a)


@pytest.mark.parametrize("kw,word", [
    (dict(decode_weights=None), "'mfma'"),                                  # bf16 weights: the message points to the bf16 mode
    (dict(decode_weights="bf16"), "'mfma'"),
    (dict(dtype=torch.float32), "bf16"),
    (dict(env={"VG_DECODE_CHAIN": "1"}), "VG_DECODE_CHAIN"),
    (dict(env={"VG_DECODE_CHAIN": "3"}), "VG_DECODE_CHAIN"),
    (dict(env={"VG_DECODE_AHEAD": "1"}), "VG_DECODE_AHEAD"),
    (dict(step=None), "step"),
    (dict(quant=[(11008, 4096, "w8", True), (4096, 11008, "w8", False), (32000, 4096, "w8", False)]), "[4096, 11008]"),      # a K the kernels do not walk
    (dict(decode_weights="mxfp4", quant=[(11008, 4096, "w4", True), (4096, 11008, "w4", False), (32000, 4096, "w8", False)]), "[4096, 11008]"),
    (dict(quant=[(13824, 5120, "w8", True)]), "[13824, 5120]"),
    (dict(projections=[(5120, 5120)]), "[5120, 5120]"),                     # the bf16 o projection
    (dict(projections=[(8192, 8192)], quant=[(28672, 8192, "w8", True), (8192, 28672, "w8", False)]), "hidden 8192"),       # the norm form
    (dict(decode_weights="mxfp4", projections=[(8192, 8192)], quant=[(28672, 8192, "w4", True)]), "4096"),
])
def test_mode_refused_with_the_reason(kw, word):
    with pytest.raises(ValueError) as e:
        _mode(**kw)
    assert word in str(e.value) and "mfma_q" in str(e.value)


def test_mode_asks_each_kernel_about_its_projections():
    seen = {"bf16": [], "w8": [], "w4": []}

    def ask(kind):
        return lambda N, K: seen[kind].append((N, K)) or True
    assert _mode(decode_weights="mxfp4", step="attention", projections=BF_PHI3, quant=Q_PHI3["mxfp4"], supported=ask("bf16"),
                 quant_supported={"w8": ask("w8"), "w4": ask("w4")}) == "mfma_q"
    assert seen == {"bf16": BF_PHI3, "w4": [(8192, 3072), (3072, 8192)], "w8": [(32064, 3072)]}
    seen = {"bf16": [], "w8": [], "w4": []}
    assert _mode(decode_weights="fp8", supported=ask("bf16"), quant_supported={"w8": ask("w8"), "w4": ask("w4")}) == "mfma_q"
    assert seen == {"bf16": BF_LLAMA, "w8": [(14336, 4096), (4096, 14336), (128256, 4096)], "w4": []}


def test_batched_route_takes_no_new_argument():
    from videoglamm_amd import prompts

    assert list(inspect.signature(prompts.batched_route).parameters) == ["B", "rope_path", "decode_weights", "chain", "routes", "env", "attn_rows",
                                                                         "w8_rows", "w4_rows", "switch"]
