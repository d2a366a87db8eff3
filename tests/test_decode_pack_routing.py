"""Where vlm.DecodeProjections routes the 13-bit rows: gate|up and down of the VALU single-row step of a bf16 model with bf16 decode
weights at Llama widths, by VG_DECODE_PACK.  Pure: no device, no library."""
from videoglamm_amd import vlm

LLAMA = dict(hidden=4096, ffn=14336, vocab=128256, qkv=6144, step="rope")
PHI3 = dict(hidden=3072, ffn=8192, vocab=32064, qkv=9216, step="attention")
ROLES = ("o", "gate_up", "down", "lm_head")


def _entries(t, rows=False):
    return tuple(t.entry(r, rows) for r in ROLES)


def test_default_routes_the_measured_shapes():
    t = vlm.DecodeProjections(None, None, env={}, **LLAMA)
    assert t.pack == {r for r, _ in vlm.DecodeProjections.PACK_DEFAULT} == {"gate_up", "down"}
    assert _entries(t) == ("decode_gemv", "decode_gemv", "decode_gemv", "linear")               # the entry point stays; run() hands it p13=
    assert _entries(t, rows=True) == ("decode_gemv_rows", "decode_gemv_rows", "decode_gemv_rows", "linear")       # the batched step stays bf16
    assert all(fmt == "bf16" for _, _, fmt, _ in t.weights()) and t.weights(quantised=True) == []


def test_knob_values():
    assert vlm.DecodeProjections("valu", "bf16", env={"VG_DECODE_PACK": "0"}, **LLAMA).pack == set()
    assert vlm.DecodeProjections("valu", "bf16", env={"VG_DECODE_PACK": "1"}, **LLAMA).pack == {"gate_up", "down"}
    t = vlm.DecodeProjections("valu", None, env={"VG_DECODE_PACK": "0"}, **LLAMA)
    assert _entries(t) == ("decode_gemv", "decode_gemv", "decode_gemv", "linear")


def test_everything_else_is_unchanged():
    for env in ({}, {"VG_DECODE_PACK": "1"}):
        assert vlm.DecodeProjections(None, None, env=env, **PHI3).pack == set()                       # Phi-3 widths
        assert vlm.DecodeProjections("mfma", None, env=env, **LLAMA).pack == set()                   # the MFMA B-row projections
        assert vlm.DecodeProjections(None, "fp8", env=env, **LLAMA).pack == set()                    # quantised decode weights
        assert vlm.DecodeProjections(None, "mxfp4", env=env, **LLAMA).pack == set()
        assert vlm.DecodeProjections("mfma_q", "fp8", env=env, **LLAMA).pack == set()
        assert vlm.DecodeProjections(None, None, env=env, pack=False, **LLAMA).pack == set()         # a model that is not bf16


class _Params:
    def w(self, name):
        return ("w", name)

    def fused(self, names, stored=None):
        return ("fused", tuple(names), stored), None

    def p13(self, names, stored=None):
        return None if names == "model.layers.3.mlp.down_proj" else ("packed", "scales", "raw")


def test_packed_operands_and_the_matrix_over_the_cap():
    P, l = _Params(), "model.layers.3."
    t = vlm.DecodeProjections(None, None, env={}, **LLAMA)
    gu = (l + "mlp.gate_proj", l + "mlp.up_proj")
    assert t.operands(P, "gate_up", l) == (("fused", gu, l + "mlp.gate_up_proj"),)
    assert t.operands(P, "gate_up", l, packed=True) == (("fused", gu, l + "mlp.gate_up_proj"), "packed", "scales", "raw")
    assert t.operands(P, "down", l, packed=True) == (("w", l + "mlp.down_proj"),)                    # Params.p13 gave None: the bf16 kernel


def test_run_hands_the_packed_rows_to_the_single_row_entry_only(monkeypatch):
    calls = []
    monkeypatch.setattr(vlm.ops, "decode_gemv", lambda x, w, **kw: calls.append(("decode_gemv", w, kw)))
    monkeypatch.setattr(vlm.ops, "decode_gemv_rows", lambda x, w, **kw: calls.append(("decode_gemv_rows", w, kw)))
    P, l = _Params(), "model.layers.3."
    t = vlm.DecodeProjections(None, None, env={}, **LLAMA)
    t.run("gate_up", False, P, l, "x", glu=True)
    t.run("down", False, P, l, "x")
    t.run("o", False, P, l, "x")
    t.run("gate_up", True, P, l, "x", glu=True)
    gu = ("fused", (l + "mlp.gate_proj", l + "mlp.up_proj"), l + "mlp.gate_up_proj")
    assert calls == [("decode_gemv", gu, dict(glu=True, p13=("packed", "scales", "raw"))),
                     ("decode_gemv", ("w", l + "mlp.down_proj"), dict(p13=None)),                   # over the cap
                     ("decode_gemv", ("w", l + "self_attn.o_proj"), {}),
                     ("decode_gemv_rows", gu, dict(glu=True))]
