"""model.inference_clips() / clips.generate_clips() on the host: the grouping, the slots' bound, which groups take the batched
step, the argument checks and refusals, the order the sampling seeds are drawn in — and, on the CPU statements of the kernels (where no group
takes the batched step), that entry b equals inference() on clip b."""
import numpy as np
import pytest
import torch

from videoglamm_amd import clips, prompts

torch.set_grad_enabled(False)


# ------------------------------------------------------------------ plan functions
def test_grouping_of_17():
    assert clips.groups(17) == [(0, 16), (16, 17)]
    assert clips.groups(16) == [(0, 16)] and clips.groups(1) == [(0, 1)] and clips.groups(0) == []
    assert clips.groups(33) == [(0, 16), (16, 32), (32, 33)]


def test_n_bound_rounding_and_max_len():
    # need = max(lens) + new + 1, rounded up to 256
    assert clips.slot_bound([99, 300, 257], 10, 1024) == 512            # 311 -> 512
    assert clips.slot_bound([245], 10, 1024) == 256                     # 256 -> 256
    assert clips.slot_bound([246], 10, 1024) == 512                     # 257 -> 512
    # similar clips share one bound (one state, one captured graph)
    assert clips.slot_bound([3361, 3300], 32, 4096) == clips.slot_bound([3350, 3200, 3400], 32, 4096) == 3584
    # the round-up never passes the decoder's length ...
    assert clips.slot_bound([1000], 10, 1024) == 1024 and clips.slot_bound([1013], 10, 1024) == 1024
    assert clips.slot_bound([900], 10, 1000) == 1000
    # ... and a clip that does not fit is refused
    with pytest.raises(ValueError):
        clips.slot_bound([1014], 10, 1024)
    # the decoder a group makes holds its bound
    for need in (1, 1024, 1025, 3394, 4097):
        L = clips.decoder_len(need)
        assert L % 1024 == 0 and L >= need and clips.slot_bound([need - 11], 10, L) <= L


def test_spliced_and_visual_rows():
    ids = torch.tensor([1, 5, 6, -200, -200, -200, -200, 9, 9])
    assert clips.spliced_rows(ids, 96) == 3 + 96 + 2
    assert clips.spliced_rows(torch.tensor([1, 2, 3]), 96) == 3
    cfg = dict(clip=dict(patch_size=14), iv2=dict(patch_size=14))
    assert clips.visual_rows(cfg, torch.empty(16, 3, 224, 224), torch.empty(16, 3, 336, 336)) == 16 * (144 + 64)
    assert clips.visual_rows(cfg, torch.empty(2, 3, 336, 336), None) == 2 * 576


def _route(**kw):
    a = dict(B=4, rope_path=True, decode_weights=None, chain=0, routes=["greedy"] * 4, env={}, attn_rows=False, w8_rows=False, w4_rows=False)
    a.update(kw)
    return prompts.batched_route(a["B"], a["rope_path"], a["decode_weights"], a["chain"], a["routes"], a["env"], attn_rows=a["attn_rows"],
                                 w8_rows=a["w8_rows"], w4_rows=a["w4_rows"], switch="VG_CLIPS_BATCHED")


def test_route_takes_the_batched_step():
    assert _route() and _route(B=2, routes=["sample_fast"] * 2) and _route(B=16, routes=["sample"] * 16)
    assert _route(rope_path=False, attn_rows=True)                      # Phi-3-mini's decode_attention rows step
    assert _route(decode_weights="fp8", w8_rows=True) and _route(decode_weights="mxfp4", w4_rows=True)
    assert _route(env={"VG_PROMPTS_BATCHED": "0"})                     # the prompts route's switch is not this route's


@pytest.mark.parametrize("kw", [
    dict(B=1, routes=["greedy"]),
    dict(B=17, routes=["greedy"] * 17),
    dict(rope_path=False),                                              # fp32, micro widths, CPU
    dict(decode_weights="fp8"), dict(decode_weights="mxfp4"),           # widths the B-row GEMVs do not cover
    dict(chain=1),
    dict(routes=["greedy", "sample_fast", "greedy", "greedy"]),
    dict(routes=["sample", "sample_fast", "sample", "sample"]),
    dict(env={"VG_CLIPS_BATCHED": "0"}),
    dict(env={"VG_DECODE_AHEAD": "1"}),
])
def test_route_falls_back_to_the_loop(kw):
    assert not _route(**kw)


def test_the_prompts_switch_is_unchanged():
    r = lambda env: prompts.batched_route(4, True, None, 0, ["greedy"] * 4, env)
    assert r({}) and r({"VG_CLIPS_BATCHED": "0"}) and not r({"VG_PROMPTS_BATCHED": "0"})


def test_as_clip():
    six = (1, 2, 3, 4, 5, 6)
    assert clips.as_clip(six) == six and clips.as_clip(list(six)) == six
    assert clips.as_clip(dict(zip(clips.CLIP_FIELDS, six))) == six
    with pytest.raises(ValueError, match=r"clips\[3\]"):
        clips.as_clip(six[:5], 3)
    with pytest.raises(ValueError, match=r"clips\[1\].*original_size_list"):
        clips.as_clip(dict(zip(clips.CLIP_FIELDS[:5], six)), 1)
    with pytest.raises(ValueError):
        clips.as_clip(torch.zeros(6))


# ------------------------------------------------------------------ the façade on the CPU statements of the kernels
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


def _clips(inp, n=3, frames=None):
    """n clips: the fixture's (its first `frames` SAM frames), and variants with other frames (one SAM frame fewer in clip 1) and other question ids"""
    base = inp["input_ids"]
    n0 = int((base == -200).nonzero().max()) + 1
    g = torch.Generator().manual_seed(11)
    out = []
    for b in range(n):
        ids = base if b == 0 else torch.cat([base[:n0], torch.randint(10, 200, (2 + b,), generator=g)])
        sam = inp["images_for_sam"][:frames]
        sam = sam if b != 1 else sam[:-1].flip(0).contiguous()
        img = inp["images"] if b == 0 else inp["images"].roll(b, 0).contiguous()
        ctx = inp["context_images"] if b == 0 else inp["context_images"].roll(b, 0).contiguous()
        out.append(([img], [ctx], [sam], ids[None], [(1024, 1024)], [inp["original_size"]]))
    return out


def same_segments(a, b):
    assert sorted(a) == sorted(b)
    for t in a:
        assert sorted(a[t]) == sorted(b[t])
        for k in a[t]:
            assert np.array_equal(a[t][k], b[t][k]), (t, k)


def _same(got, ref):
    assert len(got) == len(ref)
    for (o, s), (ro, rs) in zip(got, ref):
        assert torch.equal(o, ro) and len(s) == len(rs) == 1
        same_segments(s[0], rs[0])


@pytest.mark.parametrize("video", [False, True])
def test_each_clip_equals_its_inference(tiny, video):
    m, inp = tiny
    cl = _clips(inp, 2 if video else 3, frames=2)
    m.token_hook = lambda step, tok: m.config.seg_token_idx if step == 1 else None
    try:
        ref = [m.inference(*c, max_new_tokens=3, use_sam2_video_branch=video) for c in cl]
        # (tuples on one branch, dicts on the other)
        got = m.inference_clips(cl if video else [dict(zip(clips.CLIP_FIELDS, c)) for c in cl], max_new_tokens=3, use_sam2_video_branch=video)
    finally:
        m.token_hook = None
    _same(got, ref)
    assert len({o.shape[1] for o, _ in got}) > 1 and (len(got[0][1][0]), len(got[1][1][0])) == (2, 1)      # other prompt lengths, other frame counts


@pytest.mark.parametrize("mode", ["serial", "prefill"])
def test_hiera_start_modes(tiny, mode, monkeypatch):
    m, inp = tiny
    cl = _clips(inp, 2, frames=2)
    m.token_hook = lambda step, tok: m.config.seg_token_idx if step == 1 else None
    try:
        ref = m.inference_clips(cl, max_new_tokens=2)
        monkeypatch.setenv("VG_HIERA_START", mode)
        got = m.inference_clips(cl, max_new_tokens=2)
    finally:
        m.token_hook = None
    _same(got, ref)


def test_clip_without_seg(tiny):
    """as inference(): [{}] on the video branch, the reference's AttributeError on the framewise one"""
    m, inp = tiny
    base = inp["input_ids"]
    n0 = int((base == -200).nonzero().max()) + 1
    c = _clips(inp, 1, frames=1)[0]
    bare = c[:3] + (base[:n0][None],) + c[4:]
    m.token_hook = lambda step, tok: 7                      # never [SEG]
    try:
        ref = m.inference(*bare, max_new_tokens=2, use_sam2_video_branch=True)
        got = m.inference_clips([bare, bare], max_new_tokens=2, use_sam2_video_branch=True)
        assert got[0][1] == got[1][1] == ref[1] == [{}] and torch.equal(got[0][0], ref[0])
        with pytest.raises(AttributeError):
            m.inference_clips([bare], max_new_tokens=2)
    finally:
        m.token_hook = None


def test_refusals(tiny):
    m, inp = tiny
    cl = _clips(inp, 2)
    with pytest.raises(NotImplementedError, match="at least one clip"):
        m.inference_clips([])
    with pytest.raises(ValueError, match=r"clips\[1\]"):
        m.inference_clips([cl[0], cl[1][:5]])                                          # five fields
    with pytest.raises(ValueError, match=r"clips\[1\]"):
        m.inference_clips([cl[0], cl[1][:3] + (cl[1][3][0],) + cl[1][4:]])             # ids [L], not [1, L]
    with pytest.raises(ValueError, match=r"clips\[0\]"):
        m.inference_clips([([inp["images"]] * 2,) + cl[0][1:]])                        # two clips in one entry
    for name, val in (("capture", {}), ("stages", [])):
        setattr(m, name, val)
        try:
            with pytest.raises(NotImplementedError, match=name):
                m.inference_clips(cl)
        finally:
            setattr(m, name, None)

    class World2:
        world = 2
    m.comm = World2()
    try:
        with pytest.raises(NotImplementedError, match="one GPU"):
            m.inference_clips(cl)
    finally:
        m.comm = None


def test_seed_order(tiny, monkeypatch):
    """sampling draws B seeds from the generator in list order, before any clip runs; greedy leaves the RNG alone"""
    from videoglamm_amd import model as M
    m, inp = tiny
    cl = _clips(inp, 3, frames=2)
    seen = []

    def fake(params, cfg, towers, text, max_new_tokens, eos, token_hook=None, samplings=None, **kw):
        seen.append(samplings)
        for b in range(len(text)):
            (kw.get("before_clip") or kw.get("after_prefill"))(b)
        return [(t[2], torch.empty(0, 256)) for t in text]

    monkeypatch.setattr(clips, "generate_clips", fake)
    monkeypatch.setattr(m.sam2, "hiera_frames", lambda *a, **k: {})          # no [SEG] on the video branch: the features are never read
    gen = torch.Generator().manual_seed(123)
    want = [int(torch.empty((), dtype=torch.int64).random_(generator=gen)) for _ in range(3)]
    gen.manual_seed(123)
    m.inference_clips(cl, max_new_tokens=2, use_sam2_video_branch=True, do_sample=True, top_k=5, temperature=0.7, generator=gen)
    assert [s["seed"] for s in seen[-1]] == want and all(s["k"] == 5 and s["T"] == 0.7 for s in seen[-1])
    # the default generator: torch.manual_seed(n) + inference_clips == torch.manual_seed(n) + the B inference() calls' draws
    torch.manual_seed(77)
    ref = [M.resolve_sampling(m.generation_config, do_sample=True)["seed"] for _ in range(3)]
    torch.manual_seed(77)
    m.inference_clips(cl, max_new_tokens=2, use_sam2_video_branch=True, do_sample=True)
    assert [s["seed"] for s in seen[-1]] == ref
    # greedy: no draw
    torch.manual_seed(5)
    state = torch.get_rng_state()
    m.inference_clips(cl, max_new_tokens=2, use_sam2_video_branch=True)
    assert seen[-1] == [None] * 3 and torch.equal(torch.get_rng_state(), state)


def test_generate_clips_equals_generate_on_cpu(tiny):
    """17 clips on the CPU statements: groups of 16 + 1, every group the plain loop, every clip generate()'s result"""
    from videoglamm_amd import vlm
    m, inp = tiny
    D = m.cfg["llm"]["hidden"]
    g = torch.Generator().manual_seed(3)
    base = inp["input_ids"]
    n0 = int((base == -200).nonzero().max()) + 1
    visuals = [torch.randn(5 + b % 4, D, generator=g) * 0.5 for b in range(17)]
    text = [(None, None, torch.cat([base[:n0], torch.randint(10, 200, (b % 3,), generator=g)])) for b in range(17)]
    seg = m.config.seg_token_idx
    hook = lambda step, tok: seg if step == 1 else None
    calls = []
    got = clips.generate_clips(m.P, m.cfg, None, text, 3, None, token_hook=hook, visuals=visuals, before_clip=lambda b: calls.append(("before", b)),
                               after_prefill=lambda b: calls.append(("after", b)))
    assert calls == [(w, b) for b in range(17) for w in ("before", "after")] and len(got) == 17
    for b in (0, 5, 16):
        o, e = vlm.generate(m.P, m.cfg, None, None, None, text[b][2], 3, None, visual=visuals[b], token_hook=hook)
        assert torch.equal(got[b][0], o) and torch.equal(got[b][1], e) and e.shape[0] == 1
    assert not getattr(m.P._decoder, "_rows", None)
