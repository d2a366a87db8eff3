"""The batched multi-prompt decode on the host: which groups take it, the step buckets and the slot layout."""
import pytest

from videoglamm_amd import prompts


def _route(**kw):
    a = dict(B=4, rope_path=True, decode_weights=None, chain=0, routes=["greedy"] * 4, env={})
    a.update(kw)
    return prompts.batched_route(a["B"], a["rope_path"], a["decode_weights"], a["chain"], a["routes"], a["env"])


def test_route_llama_bf16_takes_the_batched_step():
    assert _route()
    assert _route(B=2, routes=["sample_fast"] * 2)
    assert _route(B=16, routes=["sample"] * 16)


@pytest.mark.parametrize("kw", [
    dict(B=1, routes=["greedy"]),                               # one prompt: the single-row step
    dict(B=17, routes=["greedy"] * 17),                         # more than a bucket (model.inference_prompts groups by 16)
    dict(rope_path=False),                                      # fp32, Phi-3 width (head_dim 96, window)
    dict(decode_weights="fp8"),
    dict(chain=1),                                              # VG_DECODE_CHAIN
    dict(routes=["greedy", "sample_fast", "greedy", "greedy"]),  # mixed sampling routes
    dict(routes=["sample", "sample_fast", "sample", "sample"]),
    dict(env={"VG_PROMPTS_BATCHED": "0"}),
    dict(env={"VG_DECODE_AHEAD": "1"}),
])
def test_route_keeps_the_sequential_loop(kw):
    assert not _route(**kw)


def test_buckets():
    assert [prompts.bucket(b) for b in range(1, 17)] == [2, 2, 4, 4, 8, 8, 8, 8] + [16] * 8
    with pytest.raises(ValueError):
        prompts.bucket(17)


def test_sampling_route():
    assert prompts.sampling_route(None, 8192) == "greedy"
    assert prompts.sampling_route(dict(T=1.0, k=50, p=1.0, seed=1), 8192) == "sample_fast"
    assert prompts.sampling_route(dict(T=1.0, k=0, p=0.9, seed=1), 8192) == "sample"


@pytest.mark.parametrize("P,row0", [(99, 0), (255, 0), (256, 256), (257, 256), (1700, 1536)])
def test_slot_layout(P, row0):
    r0, nb = prompts.slot_layout(P, 256, P + 40)
    assert (r0, nb) == (row0, P + 40)
    assert r0 % 256 == 0 and r0 <= P < nb
