"""The batched multi-prompt decode of the decode_attention step (Phi-3-mini width) on the host: which groups take it and the slot
layout at 128-key alignment."""
import pytest

from videoglamm_amd import prompts
from videoglamm_amd.vlm import RowsDecode


def _route(**kw):
    a = dict(B=4, rope_path=False, decode_weights=None, chain=0, routes=["greedy"] * 4, env={}, attn_rows=True)
    a.update(kw)
    return prompts.batched_route(a["B"], a["rope_path"], a["decode_weights"], a["chain"], a["routes"], a["env"], attn_rows=a["attn_rows"])


def test_route_phi3_bf16_takes_the_batched_step():
    assert _route()
    assert _route(B=2, routes=["sample_fast"] * 2)
    assert _route(B=16, routes=["sample"] * 16)
    assert _route(B=8, env={"VG_PROMPTS_BATCHED": "1", "VG_DEC_KPW_MIN": "64"})


def test_route_without_the_new_argument_is_unchanged():
    assert not prompts.batched_route(4, False, None, 0, ["greedy"] * 4, {})
    assert prompts.batched_route(4, True, None, 0, ["greedy"] * 4, {})
    assert not _route(attn_rows=False)


@pytest.mark.parametrize("kw", [
    dict(B=1, routes=["greedy"]),                               # one prompt: the single-row step
    dict(B=17, routes=["greedy"] * 17),                         # more than a bucket (model.inference_prompts groups by 16)
    dict(attn_rows=False),                                      # fp32, or a shape the B-row kernels do not cover
    dict(decode_weights="fp8"),
    dict(chain=1),                                              # VG_DECODE_CHAIN
    dict(routes=["greedy", "sample_fast", "greedy", "greedy"]),  # mixed sampling routes
    dict(routes=["sample", "sample_fast", "sample", "sample"]),
    dict(env={"VG_PROMPTS_BATCHED": "0"}),
    dict(env={"VG_DECODE_AHEAD": "1"}),
])
def test_route_keeps_the_sequential_loop(kw):
    assert not _route(**kw)


@pytest.mark.parametrize("P,row0", [(99, 0), (127, 0), (128, 128), (129, 128), (300, 256), (520, 512), (1700, 1664), (3370, 3328)])
def test_slot_layout_at_128_keys(P, row0):
    kw = RowsDecode.ATTN_KW
    assert kw == 128
    r0, nb = prompts.slot_layout(P, kw, P + 40)
    assert (r0, nb) == (row0, P + 40)
    # every 64- and 128-key split lies wholly below row0 (shared) or wholly at / above it (per slot)
    for L in (64, 128):
        assert r0 % L == 0
        for s in range(nb // L + 1):
            assert s * L + L <= r0 or s * L >= r0
