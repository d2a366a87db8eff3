"""vlm.DecodeProjections, the one table of the LLM decode step's projections: for every mode the entry point of each role in the single-row and
the B-row step, and the [N, K] / format / behind-a-norm description that decode_gemv_mode and prompts.rows_cover are asked with.  Pure: no device,
no library.  Every expected value is a literal."""
import pytest

from videoglamm_amd import vlm

# (decode_gemv, decode_weights) -> rows -> (bf16 roles: qkv and o, gate_up and down, lm_head)
TRUTH = {
    ("valu", None): {False: ("decode_gemv", "decode_gemv", "linear"), True: ("decode_gemv_rows", "decode_gemv_rows", "linear")},
    ("valu", "fp8"): {False: ("decode_gemv", "decode_gemv_w8", "decode_gemv_w8"),
                      True: ("decode_gemv_rows", "decode_gemv_w8_rows", "decode_gemv_w8_rows")},
    ("valu", "mxfp4"): {False: ("decode_gemv", "decode_gemv_w4", "decode_gemv_w8"),
                        True: ("decode_gemv_rows", "decode_gemv_w4_rows", "decode_gemv_w8_rows")},
    ("mfma", None): {False: ("decode_gemm_rows", "decode_gemm_rows", "decode_gemm_rows"),
                     True: ("decode_gemm_rows", "decode_gemm_rows", "decode_gemm_rows")},
    ("mfma_q", "fp8"): {False: ("decode_gemm_rows", "decode_gemm_w8_rows", "decode_gemm_w8_rows"),
                        True: ("decode_gemm_rows", "decode_gemm_w8_rows", "decode_gemm_w8_rows")},
    ("mfma_q", "mxfp4"): {False: ("decode_gemm_rows", "decode_gemm_w4_rows", "decode_gemm_w8_rows"),
                          True: ("decode_gemm_rows", "decode_gemm_w4_rows", "decode_gemm_w8_rows")},
}
LLAMA = dict(hidden=4096, ffn=14336, vocab=128256, qkv=6144, step="rope")
PHI3 = dict(hidden=3072, ffn=8192, vocab=32064, qkv=9216, step="attention")


@pytest.mark.parametrize("gemv,dw", sorted(TRUTH, key=str))
@pytest.mark.parametrize("rows", [False, True])
def test_entry_points_of_every_mode(gemv, dw, rows):
    bf16, mlp, head = TRUTH[(gemv, dw)][rows]
    for spelled in ({gemv, None} if gemv == "valu" else {gemv}):          # an absent decode_gemv is "valu"
        for also in (None, "bf16") if dw is None else (dw,):             # an absent decode_weights is bf16
            t = vlm.DecodeProjections(spelled, also, **PHI3)
            got = {r: t.entry(r, rows) for r in ("qkv", "o", "gate_up", "down", "lm_head")}
            assert got == dict(qkv=bf16, o=bf16, gate_up=mlp, down=mlp, lm_head=head)


def test_entries_are_names_of_ops_functions():
    import inspect
    from videoglamm_amd import ops
    for names in vlm.DecodeProjections.KERNELS.values():
        for nm in names:
            assert inspect.isfunction(getattr(ops, nm))
    assert inspect.isfunction(ops.linear)


def test_weights_of_the_mfma_mode_in_the_order_the_mode_check_is_asked():
    llama = vlm.DecodeProjections("mfma", None, **LLAMA).weights()
    assert [(N, K) for N, K, _, _ in llama] == [(4096, 4096), (14336, 4096), (4096, 14336), (128256, 4096)]
    assert all(fmt == "bf16" for _, _, fmt, _ in llama)
    phi3 = vlm.DecodeProjections("mfma", None, **PHI3).weights()
    assert [(N, K) for N, K, _, _ in phi3] == [(3072, 3072), (8192, 3072), (3072, 8192), (32064, 3072), (9216, 3072)]
    assert [norm for _, _, _, norm in phi3] == [False, True, False, False, True]             # gate|up and q|k|v run behind a norm


@pytest.mark.parametrize("dw,kind", [("fp8", "w8"), ("mxfp4", "w4")])
def test_weights_of_the_mfma_q_mode(dw, kind):
    t = vlm.DecodeProjections("mfma_q", dw, **LLAMA)
    assert t.weights(quantised=False) == [(4096, 4096, "bf16", False)]
    assert t.weights(quantised=True) == [(14336, 4096, kind, True), (4096, 14336, kind, False), (128256, 4096, "w8", False)]
    t = vlm.DecodeProjections("mfma_q", dw, **PHI3)
    assert t.weights(quantised=False) == [(3072, 3072, "bf16", False), (9216, 3072, "bf16", True)]
    assert t.weights(quantised=True) == [(8192, 3072, kind, True), (3072, 8192, kind, False), (32064, 3072, "w8", False)]
    assert t.weights() == t.weights(quantised=False)[:1] + t.weights(quantised=True) + t.weights(quantised=False)[1:]


def test_attention_width_other_than_hidden():
    t = vlm.DecodeProjections("mfma", None, hidden=4096, ffn=14336, vocab=8192, qkv=5120, attn=3072, step="attention")
    assert t.weights()[0] == (4096, 3072, "bf16", False) and t.weights()[-1] == (5120, 4096, "bf16", True)


class _Params:
    """records which stored form each role asks for"""
    def w(self, name):
        return ("w", name)

    def fused(self, names, stored=None):
        return ("fused", tuple(names), stored), None

    def fp8(self, names, stored=None):
        return ("fp8 codes", names if isinstance(names, str) else tuple(names), stored), "fp8 scales"

    def fp4(self, names, stored=None):
        return ("fp4", names if isinstance(names, str) else tuple(names), stored)


def test_operands_per_format():
    P, l = _Params(), "model.layers.3."
    qkv = (l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj")
    gu = (l + "mlp.gate_proj", l + "mlp.up_proj")
    for dw in (None, "fp8", "mxfp4"):
        t = vlm.DecodeProjections("valu", dw)
        assert t.operands(P, "qkv", l) == (("fused", qkv, l + "self_attn.qkv_proj"),)
        assert t.operands(P, "o", l) == (("w", l + "self_attn.o_proj"),)
    t = vlm.DecodeProjections("mfma", None)
    assert t.operands(P, "gate_up", l) == (("fused", gu, l + "mlp.gate_up_proj"),)
    assert t.operands(P, "down", l) == (("w", l + "mlp.down_proj"),)
    assert t.operands(P, "lm_head") == (("w", "lm_head"),)
    t = vlm.DecodeProjections("mfma_q", "fp8")
    assert t.operands(P, "gate_up", l) == (("fp8 codes", gu, l + "mlp.gate_up_proj"), "fp8 scales")
    assert t.operands(P, "down", l) == (("fp8 codes", l + "mlp.down_proj", None), "fp8 scales")
    assert t.operands(P, "lm_head") == (("fp8 codes", "lm_head", None), "fp8 scales")
    t = vlm.DecodeProjections(None, "mxfp4")
    assert t.operands(P, "gate_up", l) == (("fp4", gu, l + "mlp.gate_up_proj"),)
    assert t.operands(P, "down", l) == (("fp4", l + "mlp.down_proj", None),)
    assert t.operands(P, "lm_head") == (("fp8 codes", "lm_head", None), "fp8 scales")        # the quantised lm_head is always fp8
