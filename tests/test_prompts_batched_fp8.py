"""The batched multi-prompt decode with fp8 decode weights on the host: prompts.batched_route takes the batched step for
decode_weights="fp8" only when the B-row fp8 GEMV covers the decoder (w8_rows), and nothing else about the route moves."""
import pytest

from videoglamm_amd import prompts


def _route(**kw):
    a = dict(B=4, rope_path=True, decode_weights="fp8", chain=0, routes=["greedy"] * 4, env={}, attn_rows=False, w8_rows=True)
    a.update(kw)
    return prompts.batched_route(a["B"], a["rope_path"], a["decode_weights"], a["chain"], a["routes"], a["env"], attn_rows=a["attn_rows"],
                                 w8_rows=a["w8_rows"])


def test_fp8_takes_the_batched_step_with_the_rows_kernel():
    assert _route() is True                                     # the rope path (Llama-3-8B width)
    assert _route(rope_path=False, attn_rows=True) is True      # the decode_attention path (Phi-3-mini width)
    assert _route(B=2, routes=["sample_fast"] * 2)
    assert _route(B=16, routes=["sample"] * 16)


def test_fp8_without_the_rows_kernel_keeps_the_sequential_loop():
    assert not _route(w8_rows=False)
    assert not _route(w8_rows=False, rope_path=False, attn_rows=True)


@pytest.mark.parametrize("kw", [
    dict(B=1, routes=["greedy"]),
    dict(B=17, routes=["greedy"] * 17),
    dict(chain=1),
    dict(routes=["greedy", "sample_fast", "greedy", "greedy"]),
    dict(env={"VG_PROMPTS_BATCHED": "0"}),
    dict(env={"VG_DECODE_AHEAD": "1"}),
    dict(rope_path=False, attn_rows=False),                     # neither form of the step covers the decoder
])
def test_fp8_keeps_every_other_exclusion(kw):
    assert not _route(**kw)


def test_w8_rows_does_not_open_a_route_for_bf16():
    assert _route(decode_weights=None, w8_rows=False)
    assert _route(decode_weights="bf16", w8_rows=True)
    assert not _route(decode_weights=None, rope_path=False, attn_rows=False, w8_rows=True)


def test_calls_without_the_keyword_are_unchanged():
    r = ["greedy"] * 4
    assert prompts.batched_route(4, True, None, 0, r, {})
    assert prompts.batched_route(4, False, None, 0, r, {}, True)
    assert prompts.batched_route(4, False, None, 0, r, {}, attn_rows=True)
    assert not prompts.batched_route(4, True, "fp8", 0, r, {})
    assert not prompts.batched_route(4, False, "fp8", 0, r, {}, attn_rows=True)
