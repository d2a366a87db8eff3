"""Which projection launches one eager decode step makes, in order and on which weight: the single-row step of LlamaDecoder and the B = 2 step of
RowsDecode, in every (decode_gemv, decode_weights) mode, against the tensors Params holds for that layer and role.  The per-kernel call counts of
the mode tests cannot see a role that was handed another role's weight, or two roles in the wrong order; this does."""
import pytest
import torch

import test_prompts_batched_gpu as llama
import test_prompts_batched_phi3_gpu as phi3

torch.set_grad_enabled(False)
pytestmark = pytest.mark.gpu

NAMES = ["decode_gemv", "decode_gemv_w8", "decode_gemv_w4", "decode_gemv_rows", "decode_gemv_w8_rows", "decode_gemv_w4_rows",
         "decode_gemm_rows", "decode_gemm_w8_rows", "decode_gemm_w4_rows", "linear"]
# (decode_gemv, decode_weights) -> rows -> entry of (the bf16 roles o and q|k|v, gate_up and down, lm_head)
ENTRIES = {
    ("valu", None): {False: ("decode_gemv", "decode_gemv", "linear"), True: ("decode_gemv_rows", "decode_gemv_rows", "linear")},
    ("valu", "fp8"): {False: ("decode_gemv", "decode_gemv_w8", "decode_gemv_w8"),
                      True: ("decode_gemv_rows", "decode_gemv_w8_rows", "decode_gemv_w8_rows")},
    ("valu", "mxfp4"): {False: ("decode_gemv", "decode_gemv_w4", "decode_gemv_w8"),
                        True: ("decode_gemv_rows", "decode_gemv_w4_rows", "decode_gemv_w8_rows")},
    ("mfma", None): {r: ("decode_gemm_rows", "decode_gemm_rows", "decode_gemm_rows") for r in (False, True)},
    ("mfma_q", "fp8"): {r: ("decode_gemm_rows", "decode_gemm_w8_rows", "decode_gemm_w8_rows") for r in (False, True)},
    ("mfma_q", "mxfp4"): {r: ("decode_gemm_rows", "decode_gemm_w4_rows", "decode_gemm_w8_rows") for r in (False, True)},
}
S = 40      # prefilled rows; the recorded steps run at positions 40 and 41


def _stored(P, dw, names, stored=None):
    """data_ptr of the tensor the kernels stream for a weight held as dw"""
    if dw == "fp8":
        return P.fp8(names, stored=stored)[0].data_ptr()
    if dw == "mxfp4":
        return P.fp4(names, stored=stored).data_ptr()
    return (P.w(names) if isinstance(names, str) else P.fused(names, stored=stored)[0]).data_ptr()


def _want(P, n_layers, gemv, dw, rows, qkv):
    """(entry, weight pointer, glu, norm, residual) per launch: [qkv], o, gate_up, down per layer, then the lm_head"""
    bf16, mlp, head = ENTRIES[(gemv, dw)][rows]
    seq = []
    for i in range(n_layers):
        l = f"model.layers.{i}."
        if qkv:
            seq.append((bf16, _stored(P, None, [l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj"], l + "self_attn.qkv_proj"),
                        False, True, False))
        seq.append((bf16, _stored(P, None, l + "self_attn.o_proj"), False, False, True))
        seq.append((mlp, _stored(P, dw, [l + "mlp.gate_proj", l + "mlp.up_proj"], l + "mlp.gate_up_proj"), True, True, False))
        seq.append((mlp, _stored(P, dw, l + "mlp.down_proj"), False, False, True))
    seq.append((head, _stored(P, "fp8" if dw else None, "lm_head"), False, False, False))
    return seq


def _record(ops, log):
    mp = pytest.MonkeyPatch()
    for nm in NAMES:
        def wrapped(x, w, *a, _nm=nm, _fn=getattr(ops, nm), **kw):
            log.append((_nm, w.data_ptr(), bool(kw.get("glu")), kw.get("norm_w") is not None, kw.get("residual") is not None))
            return _fn(x, w, *a, **kw)
        mp.setattr(ops, nm, wrapped)
    return mp


@pytest.mark.parametrize("model,gemv,dw", [("llama",) + k for k in sorted(ENTRIES, key=str)] + [("phi3", "valu", None), ("phi3", "mfma_q", "mxfp4")])
def test_each_role_launches_on_its_own_weight_in_order(cuda, model, gemv, dw):
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder, RowsDecode
    P, cfg, _ = (phi3 if model == "phi3" else llama)._llm(cuda)
    c = dict(cfg["llm"], decode_gemv=gemv)
    if dw:
        c["decode_weights"] = dw
    dec = LlamaDecoder(P, c, 1024, use_graph=False)
    assert dec.rope_path == (model == "llama") and dec.fused_decode
    x = (torch.randn(S, c["hidden"], generator=torch.Generator().manual_seed(11)) * 0.5).to(torch.bfloat16).to(cuda)
    dec.reset()
    dec.next_token(dec.forward(x)[-1:])
    single, batched = [], []
    mp = _record(ops, single)
    try:
        dec.decode_step()                                  # the single-row step at position S
    finally:
        mp.undo()
    rows = RowsDecode(dec, 2, 0, 64)                       # two rows that continue from the decoder's state at position S + 1
    for b in range(2):
        rows.load_row(b, S, S + 1)
    mp = _record(ops, batched)
    try:
        rows.decode_step()
    finally:
        mp.undo()
    torch.cuda.synchronize()
    assert rows.attn_rows == (model == "phi3") and not rows.graphs and not dec.graphs
    assert single == _want(P, c["num_layers"], gemv, dw, False, qkv=model == "phi3")
    assert batched == _want(P, c["num_layers"], gemv, dw, True, qkv=model == "phi3")
    assert int(rows.pos[0]) == int(rows.pos[1]) == S + 2 and int(rows.tok[0]) == int(rows.tok[1])      # equal rows, equal tokens
