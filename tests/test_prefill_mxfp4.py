"""cfg["llm"]["prefill_gemm"] = "mxfp4" / cfg["llm"]["dense_mlp"] = "drop": the pure validation (vlm.prefill_gemm_mode) and Params.drop, on the CPU."""
import pytest
import torch

from videoglamm_amd.params import Params
from videoglamm_amd.vlm import prefill_gemm_mode

BF = torch.bfloat16


def test_mxfp4_mode_resolves():
    assert prefill_gemm_mode("mxfp4", None, None, BF, 4096, 14336) == ("mxfp4", False)
    assert prefill_gemm_mode("mxfp4", "fp8", "keep", BF, 3072, 8192) == ("mxfp4", False)          # independent of decode_weights, as "fp8" is
    assert prefill_gemm_mode("mxfp4", "mxfp4", "drop", BF, 8192, 14336) == ("mxfp4", True)


@pytest.mark.parametrize("decode_weights", [None, "bf16", "fp8", "mxfp4"])
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_existing_combinations_resolve_as_before(decode_weights, dtype):
    """"fp8" stays the fp8 prefill, everything else the dense prefill of the model dtype — whatever the widths or the dtype (the fp8 mode's own
    bf16 assertion stays in the decoder)"""
    assert prefill_gemm_mode("fp8", decode_weights, None, dtype, 4096, 14336) == ("fp8", False)
    for value in (None, "bf16", "anything"):
        assert prefill_gemm_mode(value, decode_weights, None, dtype, 2048, 5632) == (None, False)
        assert prefill_gemm_mode(value, decode_weights, "keep", dtype, 2048, 5632) == (None, False)


def test_refusals():
    with pytest.raises(ValueError, match="needs a bf16 model"):
        prefill_gemm_mode("mxfp4", "mxfp4", None, torch.float32, 4096, 14336)
    with pytest.raises(ValueError, match="no packed MXFP4 row of length hidden = 2048"):
        prefill_gemm_mode("mxfp4", None, None, BF, 2048, 8192)
    with pytest.raises(ValueError, match="ffn = 11008"):
        prefill_gemm_mode("mxfp4", None, None, BF, 4096, 11008)
    with pytest.raises(ValueError, match=r"the decode step \(decode_weights = 'fp8'\) still reads the dense MLP weights"):
        prefill_gemm_mode("mxfp4", "fp8", "drop", BF, 4096, 14336)
    with pytest.raises(ValueError, match=r"the decode step \(decode_weights = None\) still reads"):
        prefill_gemm_mode("mxfp4", None, "drop", BF, 4096, 14336)
    with pytest.raises(ValueError, match=r"the prefill \(prefill_gemm = 'fp8'\) still reads the dense MLP weights"):
        prefill_gemm_mode("fp8", "mxfp4", "drop", BF, 4096, 14336)
    with pytest.raises(ValueError, match=r"the prefill \(prefill_gemm = None\) still reads"):
        prefill_gemm_mode(None, "mxfp4", "drop", BF, 4096, 14336)
    with pytest.raises(ValueError, match="'keep' \\(default\\) or 'drop'"):
        prefill_gemm_mode("mxfp4", "mxfp4", "yes", BF, 4096, 14336)


def _sd(stored):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(BF)      # noqa: E731
    sd = {"l.mlp.down_proj.weight": r(16, 3072), "l.self_attn.o_proj.weight": r(16, 16), "l.norm.weight": r(16)}
    if stored:
        sd["l.mlp.gate_up_proj.weight"] = r(16, 3072)
    else:
        sd["l.mlp.gate_proj.weight"], sd["l.mlp.up_proj.weight"] = r(8, 3072), r(8, 3072)
    return sd


@pytest.mark.parametrize("stored", [False, True], ids=["llama", "phi3"])
def test_params_drop(stored):
    P = Params(_sd(stored), "cpu", BF)
    gu, st, down = ["l.mlp.gate_proj", "l.mlp.up_proj"], "l.mlp.gate_up_proj", "l.mlp.down_proj"
    f_gu, f_down = P.fp4(gu, stored=st), P.fp4(down)
    assert f_gu.shape == (16, 128 + 1536) and f_gu.dtype == torch.uint8
    keep_gu, keep_down = f_gu.clone(), f_down.clone()
    P.t(down + ".weight")                                    # a dense device copy under another cache key
    P.drop(gu + [st, down])
    assert not any(k.startswith("l.mlp.") for k in P.sd)
    assert not any(key[0] in ("w", "fused", "t") and "mlp" in str(key) for key in P._c)
    # the packed rows survive and are served from the cache
    assert P.fp4(gu, stored=st) is f_gu and P.fp4(down) is f_down
    assert torch.equal(f_gu, keep_gu) and torch.equal(f_down, keep_down)
    # dense access raises and says why
    with pytest.raises(KeyError, match="dense weight was dropped"):
        P.w(down)
    with pytest.raises(KeyError, match="dense weight was dropped"):
        P.fused(gu, stored=st)
    with pytest.raises(KeyError, match="dense weight was dropped"):
        P.fp8(down)
    # untouched names still load
    assert P.w("l.self_attn.o_proj").shape == (16, 16) and P.f32("l.norm.weight").dtype == torch.float32
    P.drop(gu + [st, down])                                   # a second decoder on the same Params: nothing left to do, nothing breaks
    assert P.fp4(down) is f_down
