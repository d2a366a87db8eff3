"""model.inference_prompts() on the CPU statements of the kernels: several prompts about one clip give, prompt by prompt, what
inference() gives for that prompt alone — ids, masks and [SEG] embeddings — on both SAM2 branches; plus the refusals and the edge cases
(empty suffix, a prompt without [SEG], more than 16 prompts)."""
import numpy as np
import pytest
import torch

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def tiny():
    import _cpu_ops
    from test_oracle_e2e import e2e_setup
    from videoglamm_amd import _lib, ops
    from videoglamm_amd.model import VideoGLaMMForCausalLM

    with pytest.MonkeyPatch.context() as mp:
        for name in _cpu_ops.ALL:
            if hasattr(ops, name):
                mp.setattr(ops, name, getattr(_cpu_ops, name))
        mp.setattr(_lib, "load", lambda: None)
        fx, sd, cfg, inp = e2e_setup()
        m = VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.float32, device="cpu")
        yield m, inp


def prompts(inp):
    """the fixture's ids, two variants with other question ids, and the prefix alone (empty suffix)"""
    base = inp["input_ids"]
    n0 = int((base == -200).nonzero().max()) + 1
    return [base, torch.cat([base[:n0], torch.tensor([84, 12, 99, 150, 7])]), torch.cat([base[:n0], torch.tensor([200, 201, 202])]), base[:n0]]


def clip(inp):
    return [inp["images"]], [inp["context_images"]], [inp["images_for_sam"]]


def one(m, inp, ids, n, video):
    m.capture = {}
    try:
        out, seg = m.inference(*clip(inp), ids[None], [(1024, 1024)], [inp["original_size"]], max_new_tokens=n, use_sam2_video_branch=video)
        return out, seg[0], m.capture["emb"]
    finally:
        m.capture = None


def many(m, inp, ids_list, n, video, capture=False):
    m.capture = {} if capture else None
    try:
        out, segs = m.inference_prompts(*clip(inp), ids_list, [(1024, 1024)], [inp["original_size"]], max_new_tokens=n, use_sam2_video_branch=video)
        return out, segs, m.capture
    finally:
        m.capture = None


def same_segments(a, b):
    assert sorted(a) == sorted(b)
    for t in a:
        assert sorted(a[t]) == sorted(b[t])
        for k in a[t]:
            assert np.array_equal(a[t][k], b[t][k]), (t, k)


def seg_hook(seg):
    return lambda step, tok: seg if step == 1 else None


@pytest.mark.parametrize("video", [False, True])
def test_each_prompt_equals_its_inference(tiny, video):
    from test_oracle_e2e import SEAM_TOL
    m, inp = tiny
    m.token_hook = seg_hook(m.config.seg_token_idx)
    try:
        P = prompts(inp)[:3]
        ref = [one(m, inp, ids, 2, video) for ids in P]
        out, segs, _ = many(m, inp, P, 2, video)            # the default (thresholded-on-device) mask path
        _, segs_c, cap = many(m, inp, P, 2, video, capture=True)
    finally:
        m.token_hook = None
    assert len(out) == len(segs) == 3
    for b, (o, s, e) in enumerate(ref):
        assert out[b].shape == (1, P[b].numel() + 2) and torch.equal(out[b], o)
        same_segments(segs[b], s)
        same_segments(segs_c[b], s)
        assert cap["emb"][b].shape == e.shape and e.shape[0] >= 1
        torch.testing.assert_close(cap["emb"][b], e, **SEAM_TOL)


def test_empty_suffix_and_no_seg(tiny):
    """the prefix alone (its first token comes from the prefix's last row) next to prompts that emit no [SEG]: those get {} on either branch,
    the fixture's prompt (all [SEG]) is unaffected"""
    m, inp = tiny
    P = prompts(inp)
    for video in (False, True):
        ref = one(m, inp, P[0], 2, video)
        out, segs, _ = many(m, inp, [P[1], P[0], P[3]], 2, video)
        assert torch.equal(out[1], ref[0]) and segs[0] == {} and segs[2] == {}
        same_segments(segs[1], ref[1])
    alone, _ = m.inference(*clip(inp), P[3][None], [(1024, 1024)], [inp["original_size"]], max_new_tokens=2, use_sam2_video_branch=True)
    assert torch.equal(out[2], alone) and out[2].shape[1] == P[3].numel() + 2


def test_more_than_16_prompts_run_in_groups(tiny):
    m, inp = tiny
    P = prompts(inp)
    ids = [P[b % 3 + 1] for b in range(17)]
    out, segs, _ = many(m, inp, ids, 1, False)
    a, sa, _ = many(m, inp, ids[:16], 1, False)
    b, sb, _ = many(m, inp, ids[16:], 1, False)
    assert len(out) == 17 and all(torch.equal(x, y) for x, y in zip(out, a + b))
    for x, y in zip(segs, sa + sb):
        same_segments(x, y)


def test_refusals(tiny):
    m, inp = tiny
    P = prompts(inp)
    with pytest.raises(ValueError, match=r"input_ids_list\[1\]"):
        many(m, inp, [P[0], torch.cat([torch.tensor([2]), P[1][1:]])], 1, False)        # other ids before the visual block
    with pytest.raises(ValueError, match=r"input_ids_list\[2\]"):
        many(m, inp, [P[0], P[1], torch.tensor([1, 5, 6, 84])], 1, False)                # no visual placeholder
    with pytest.raises(NotImplementedError):
        many(m, inp, [], 1, False)

    class World2:
        world = 2
    m.comm = World2()
    try:
        with pytest.raises(NotImplementedError):
            many(m, inp, P[:2], 1, False)
    finally:
        m.comm = None


@pytest.mark.parametrize("mode", ["serial", "prefill"])
def test_hiera_start_modes(tiny, mode, monkeypatch):
    """VG_HIERA_START is honoured as by inference(): the same results, and "serial" leaves the per-stage marks"""
    m, inp = tiny
    P = prompts(inp)[:2]
    m.token_hook = seg_hook(m.config.seg_token_idx)
    try:
        ref = many(m, inp, P, 2, False)
        monkeypatch.setenv("VG_HIERA_START", mode)
        m.stages = []
        got = many(m, inp, P, 2, False)
        names = [n for n, _ in m.stages]
    finally:
        m.token_hook, m.stages = None, None
    assert all(torch.equal(a, b) for a, b in zip(got[0], ref[0]))
    for a, b in zip(got[1], ref[1]):
        same_segments(a, b)
    assert names[-4:] == ["towers", "prefill", "decode", "mask_decode"]
    assert (names[:2] == ["begin", "hiera_fpn"]) == (mode == "serial")
