"""Clip-batched generation on the HIP kernels: the B-row decode step with row0 = 0 — every key / value row of a row in its own
slot, nothing read from the decoder's cache — gives each row the bits of the single-row kernels; clips.generate_clips() returns per clip exactly
what vlm.generate() returns for it; model.inference_clips() returns per clip exactly what model.inference() returns, ids and masks pixel for pixel.
The 2-layer decoders (Llama-3-8B and Phi-3-mini width, vocab 8192) are those of the batched multi-prompt tests; the visual blocks are synthetic."""
import numpy as np
import pytest
import torch

import test_prompts_batched_gpu as llama
import test_prompts_batched_phi3_gpu as phi3
from test_e2e_fp8_gpu import _cfg

torch.set_grad_enabled(False)

pytestmark = pytest.mark.gpu

POSITIONS = [99, 255, 256, 257, 300]          # both sides of a 128 edge (99 | 255) and of a 256-key block edge (255 | 256 | 257), and past it


# ------------------------------------------------------------------ kernels with row0 = 0, row by row against the single-row kernels
def test_qkv_rope_and_attention_rows_with_row0_zero(cuda):
    """q|k|v + RoPE + append and the attention, rows at POSITIONS mixed in one batch, each in its own slot from row 0 on; the shared cache
    handed to the kernels holds other values and must not be read: bit-equal to the single-row kernels on a decoder cache holding that row's slot"""
    from videoglamm_amd import ops
    P, cfg, _ = llama._llm(cuda)
    c = cfg["llm"]
    dec = llama._decoder(P, cfg, 1024)
    H, Hkv, hd = dec.H, dec.Hkv, dec.hd
    B, n_bound = len(POSITIONS), 512
    g = torch.Generator().manual_seed(12)
    other_k = torch.randn(1024, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    other_v = torch.randn(1024, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    ks = torch.randn(B, n_bound, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    vs = torch.randn(B, n_bound, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    ks0, vs0 = ks.clone(), vs.clone()
    x = (torch.randn(B, c["hidden"], generator=g) * 2).to(torch.bfloat16).to(cuda)
    l = "model.layers.1."
    wqkv, _ = P.fused([l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj"], stored=l + "self_attn.qkv_proj")
    nw = P.f32(l + "input_layernorm.weight")
    pos_dev = torch.tensor(POSITIONS, dtype=torch.int32, device=cuda)
    rope_cs = torch.stack([torch.cat([dec.cos[p], dec.sin[p]]) for p in POSITIONS]).contiguous()
    q = ops.decode_qkv_rope_rows(x, wqkv, nw, c["rms_eps"], ks, vs, 0, rope_cs, pos_dev, H, Hkv, hd)
    ws = ops.decode_attention2_rows_workspace(H, Hkv, hd, n_bound, dec.kpw2, B, cuda)
    o = ops.decode_attention2_rows(q, other_k, other_v, ks, vs, 0, H, Hkv, hd, pos_dev, n_bound, hd ** -0.5, ws, keys_per_wg=dec.kpw2)
    o2 = ops.decode_attention2_rows(q, other_k, other_v, ks, vs, 0, H, Hkv, hd, pos_dev, n_bound, hd ** -0.5, ws, keys_per_wg=dec.kpw2)
    assert torch.equal(o, o2)                                   # the self-resetting counters
    ws1 = ops.decode_attention_workspace(H, Hkv, hd, 1024, cuda)
    for r, p in enumerate(POSITIONS):
        kc = torch.zeros(1024, Hkv, hd, dtype=torch.bfloat16, device=cuda)
        vc = torch.zeros_like(kc)
        kc[:n_bound], vc[:n_bound] = ks0[r], vs0[r]
        p1 = torch.tensor([p], dtype=torch.int32, device=cuda)
        q1 = ops.decode_qkv_rope(x[r:r + 1].contiguous(), wqkv, nw, c["rms_eps"], kc, vc, rope_cs[r].contiguous(), p1, H, Hkv, hd)
        assert torch.equal(q[r:r + 1], q1)
        assert torch.equal(ks[r], kc[:n_bound]) and torch.equal(vs[r], vc[:n_bound])          # the appended row, and nothing else moved
        assert not torch.equal(ks[r, p], ks0[r, p])
        o1 = ops.decode_attention2(q1, kc, vc, H, Hkv, hd, p1, hd ** -0.5, ws1, keys_per_wg=dec.kpw2)
        assert torch.equal(o[r:r + 1], o1), p


@pytest.mark.parametrize("window", [0, 200])
@pytest.mark.parametrize("kpw", ["split", "64", "128"])
def test_phi3_attention_rows_with_row0_zero(cuda, window, kpw):
    """vg_decode_attention_rows (RoPE + append + attention) with row0 = 0, rows at POSITIONS mixed in one batch, on 64- and 128-key splits within
    one launch ("split": rows from position 256 on take 128), against vg_decode_attention on a cache holding that row's slot"""
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = phi3._llm(cuda)
    dec = LlamaDecoder(P, cfg["llm"], 1024)
    H, Hkv, hd = dec.H, dec.Hkv, dec.hd
    B, n_bound = len(POSITIONS), 512
    g = torch.Generator().manual_seed(31 + window)
    kpw_min = {"split": 256, "64": 8192, "128": 0}[kpw]
    other_k = torch.randn(1024, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    other_v = torch.randn(1024, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    ks = torch.randn(B, n_bound, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    vs = torch.randn(B, n_bound, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    ks0, vs0, ok0, ov0 = ks.clone(), vs.clone(), other_k.clone(), other_v.clone()
    qkv = torch.randn(B, (H + 2 * Hkv) * hd, generator=g).to(torch.bfloat16).to(cuda)
    pos_dev = torch.tensor(POSITIONS, dtype=torch.int32, device=cuda)
    ws = ops.decode_attention_rows_workspace(H, Hkv, hd, n_bound, B, cuda)
    args = (qkv, other_k, other_v, ks, vs, 0, dec.cos, dec.sin, H, Hkv, hd, pos_dev, n_bound, hd ** -0.5, ws)
    o = ops.decode_attention_rows(*args, window=window, kpw_min=kpw_min)
    o2 = ops.decode_attention_rows(*args, window=window, kpw_min=kpw_min)
    assert torch.equal(o, o2)
    assert torch.equal(other_k, ok0) and torch.equal(other_v, ov0)
    ws1 = ops.decode_attention_workspace(H, Hkv, hd, 1024, cuda)
    for r, p in enumerate(POSITIONS):
        kc = torch.zeros(1024, Hkv, hd, dtype=torch.bfloat16, device=cuda)
        vc = torch.zeros_like(kc)
        kc[:n_bound], vc[:n_bound] = ks0[r], vs0[r]
        p1 = torch.tensor([p], dtype=torch.int32, device=cuda)
        o1 = ops.decode_attention(qkv[r:r + 1].contiguous(), kc, vc, dec.cos, dec.sin, H, Hkv, hd, p1, hd ** -0.5, ws1, window=window,
                                  keys_per_wg=128 if p >= kpw_min else 0)
        assert torch.equal(o[r:r + 1], o1), p
        assert torch.equal(ks[r], kc[:n_bound]) and torch.equal(vs[r], vc[:n_bound]), p


# ------------------------------------------------------------------ generate_clips against generate() per clip
NVIS = [96, 252, 253, 254, 255, 256, 257, 300]


def _llm(cuda, model="llama", decode_weights=None):
    P, cfg, _ = (phi3 if model == "phi3" else llama)._llm(cuda)
    if decode_weights:
        cfg = dict(cfg, llm=dict(cfg["llm"], decode_weights=decode_weights))
    return P, cfg


def _make(cfg, cuda, n, seed=0, first=0):
    """n clips (None, None, ids) + their synthetic visual blocks: nvis cycles through NVIS from `first`, the prompt's tail is 0..9 ids long"""
    g = torch.Generator().manual_seed(100 + seed)
    head = torch.tensor([1, 5, 6, -200, -200, -200, -200])
    D = cfg["llm"]["hidden"]
    text, visuals = [], []
    for b in range(n):
        text.append((None, None, torch.cat([head, torch.randint(10, 8000, ((3 * b + 4 + seed) % 10,), generator=g)])))
        visuals.append((torch.randn(NVIS[(first + b) % len(NVIS)], D, generator=g) * 0.5).to(torch.bfloat16).to(cuda))
    return text, visuals


def _alone(P, cfg, text, visuals, n, eos=None, hook=None, samplings=None, traces=None):
    from videoglamm_amd import vlm
    out = []
    for b, (_, _, ids) in enumerate(text):
        o, e = vlm.generate(P, cfg, None, None, None, ids, n, eos, visual=visuals[b], token_hook=hook,
                            trace=None if traces is None else traces[b], sampling=None if samplings is None else samplings[b])
        out.append((o, e.clone()))
    return out


def _batched(P, cfg, text, visuals, n, eos=None, hook=None, samplings=None, traces=None, **kw):
    from videoglamm_amd.clips import generate_clips
    return generate_clips(P, cfg, None, text, n, eos, token_hook=hook, samplings=samplings, traces=traces, visuals=visuals, **kw)


def _same(got, ref):
    assert len(got) == len(ref)
    for b, ((o, e), (ro, re)) in enumerate(zip(got, ref)):
        assert torch.equal(o, ro), (b, o.tolist(), ro.tolist())
        assert e.shape == re.shape and torch.equal(e, re), b


def _rows(P):
    (key, rows), = P._decoder._rows.items()
    assert rows.row0 == 0 and key == (rows.B, 0, rows.n_bound) and rows.dec is P._decoder
    return rows


def _sampling(mode, B):
    if mode == "greedy":
        return None
    return [dict(T=0.8 + 0.1 * (b % 3), k=20 if mode == "k20" else 0, p=0.9, seed=100 + b) for b in range(B)]


SEG_HOOK = lambda seg: (lambda step, tok: seg if step in (1, 4) else None)      # noqa: E731  a [SEG] from the prefill's row and from a decode row


@pytest.mark.parametrize("mode", ["greedy", "k20", "k0"])
@pytest.mark.parametrize("B", [2, 5, 16])
def test_generate_clips_equals_generate(cuda, B, mode):
    P, cfg = _llm(cuda)
    text, visuals = _make(cfg, cuda, B, seed=B)
    hook = SEG_HOOK(cfg["seg_token_idx"])
    sp = _sampling(mode, B)
    ta, tb = [{} for _ in range(B)], [{} for _ in range(B)]
    ref = _alone(P, cfg, text, visuals, 9, hook=hook, samplings=sp, traces=ta)
    calls = []
    got = _batched(P, cfg, text, visuals, 9, hook=hook, samplings=sp, traces=tb, before_clip=lambda b: calls.append(("before", b)),
                   after_prefill=lambda b: calls.append(("after", b)))
    _same(got, ref)
    # before_clip(b) ahead of clip b's prefill, after_prefill(b) behind it, clip by clip, and all of them before the group's decode
    assert ta == tb and calls == [(w, b) for b in range(B) for w in ("before", "after")]
    assert all(e.shape == (2, 256) for _, e in got)
    rows = _rows(P)
    assert rows.B == (2 if B == 2 else 8 if B == 5 else 16) and rows.steps == 8
    assert rows.route == {"greedy": "greedy", "k20": "sample_fast", "k0": "sample"}[mode]
    assert len({t[2].numel() - 4 + v.shape[0] for t, v in zip(text, visuals)}) > B // 2               # the rows sit at different positions


@pytest.mark.parametrize("model,dw", [("phi3", None), ("llama", "fp8"), ("llama", "mxfp4")])
def test_other_decoders(cuda, model, dw):
    """the Phi-3-mini-width decode_attention rows step, and fp8 / mxfp4 decode weights: greedy and sampled (k = 20)"""
    P, cfg = _llm(cuda, model, dw)
    B = 5
    text, visuals = _make(cfg, cuda, B, seed=2, first=1)
    hook = SEG_HOOK(cfg["seg_token_idx"])
    for mode in ("greedy", "k20"):
        sp = _sampling(mode, B)
        ref = _alone(P, cfg, text, visuals, 8, hook=hook, samplings=sp)
        got = _batched(P, cfg, text, visuals, 8, hook=hook, samplings=sp)
        _same(got, ref)
    rows = _rows(P)
    dec = P._decoder
    assert rows.B == 8 and rows.attn_rows == (model == "phi3") and dec.w8 == (dw == "fp8") and dec.w4 == (dw == "mxfp4")
    assert sorted(rows.graphs) == ["greedy", "sample_fast"]


def test_eos_at_different_steps(cuda):
    P, cfg = _llm(cuda)
    B = 6
    text, visuals = _make(cfg, cuda, B, seed=4)
    free = _alone(P, cfg, text, visuals, 10)
    # every clip's own token at steps 1..6 as its EOS: the clips stop at different steps
    eos = sorted({int(o[t[2].numel() + 1 + b % 6]) for b, ((o, _), t) in enumerate(zip(free, text))})
    ref = _alone(P, cfg, text, visuals, 10, eos=eos)
    got = _batched(P, cfg, text, visuals, 10, eos=eos)
    _same(got, ref)
    gen = [o.numel() - t[2].numel() for (o, _), t in zip(got, text)]
    assert len(set(gen)) > 1
    rows = _rows(P)
    assert rows.steps == max(gen) - 1 and rows.steps < sum(gen) - len(gen)           # the longest clip's steps, not their sum


def test_seventeen_clips_in_groups_of_sixteen(cuda):
    P, cfg = _llm(cuda)
    text, visuals = _make(cfg, cuda, 17, seed=6)
    hook = SEG_HOOK(cfg["seg_token_idx"])
    ref = _alone(P, cfg, text, visuals, 8, hook=hook)
    P._decoder._rows = {}
    got = _batched(P, cfg, text, visuals, 8, hook=hook)
    _same(got, ref)
    rows = _rows(P)
    assert rows.B == 16 and rows.steps == 7              # the 17th clip ran the single-row loop


def test_route_taken_and_the_switch(cuda, monkeypatch):
    from videoglamm_amd import clips
    P, cfg = _llm(cuda)
    text, visuals = _make(cfg, cuda, 3, seed=7)
    monkeypatch.setenv("VG_CLIPS_BATCHED", "0")
    off = _batched(P, cfg, text, visuals, 8)
    assert not getattr(P._decoder, "_rows", None)
    _same(off, _alone(P, cfg, text, visuals, 8))
    monkeypatch.setenv("VG_CLIPS_BATCHED", "1")
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")         # the prompts route's switch is not this route's
    on = _batched(P, cfg, text, visuals, 8)
    _same(on, off)
    rows = _rows(P)
    lens = [clips.spliced_rows(t[2], v.shape[0]) for t, v in zip(text, visuals)]
    assert rows.B == 4 and rows.n_bound == clips.slot_bound(lens, 8, P._decoder.max_len) == 512 and rows.steps == 7
    assert rows.ks[0].shape[:2] == (4, 512) and rows.start_pos[:3] == lens and rows.start_pos[3] == 0
    # one clip, one new token, mixed sampling routes: the loop
    steps = rows.steps
    _same(_batched(P, cfg, text[:1], visuals[:1], 8), off[:1])
    _batched(P, cfg, text, visuals, 1)
    sp = [None, dict(T=1.0, k=20, p=0.9, seed=1), dict(T=1.0, k=0, p=0.9, seed=2)]
    _same(_batched(P, cfg, text, visuals, 8, samplings=sp), _alone(P, cfg, text, visuals, 8, samplings=sp))
    assert rows.steps == steps


def test_graph_replay_equals_eager(cuda):
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg = _llm(cuda)
    text, visuals = _make(cfg, cuda, 5, seed=8)
    hook = SEG_HOOK(cfg["seg_token_idx"])
    sp = _sampling("k20", 5)
    a = _batched(P, cfg, text, visuals, 8, hook=hook) + _batched(P, cfg, text, visuals, 8, hook=hook, samplings=sp)
    assert sorted(_rows(P).graphs) == ["greedy", "sample_fast"]
    P._decoder = LlamaDecoder(P, cfg["llm"], 1024, use_graph=False)
    b = _batched(P, cfg, text, visuals, 8, hook=hook) + _batched(P, cfg, text, visuals, 8, hook=hook, samplings=sp)
    assert not _rows(P).graphs
    _same(a, b)


def test_second_call_on_the_reused_state(cuda):
    """other clips — shorter ones in the slots that held longer ones, fewer of them — on the same RowsDecode: no stale slot row leaks"""
    P, cfg = _llm(cuda)
    hook = SEG_HOOK(cfg["seg_token_idx"])
    text, visuals = _make(cfg, cuda, 7, seed=9, first=7)               # nvis 300, 96, 252, ...
    _same(_batched(P, cfg, text, visuals, 9, hook=hook), _alone(P, cfg, text, visuals, 9, hook=hook))
    rows = _rows(P)
    text2, visuals2 = _make(cfg, cuda, 5, seed=10, first=1)            # nvis 96 in the slot that held 300 rows, ...
    ref = _alone(P, cfg, text2, visuals2, 9, hook=hook)
    got = _batched(P, cfg, text2, visuals2, 9, hook=hook)
    assert _rows(P) is rows and rows.steps == 16 and len(rows.graphs) == 1
    _same(got, ref)


# ------------------------------------------------------------------ the façade
def _micro(cuda):
    """the micro model with a Llama-width LLM (test_prompts_batched_mxfp4_gpu.py::_micro), three clips with other frames, frame counts and prompts"""
    from videoglamm_amd import synth
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    cfg = _cfg()
    sd = synth.device_state_dict(synth.manifest(cfg), cuda, torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    clips = []
    for te, T, n, hw in ((4, 3, 20, (48, 64)), (8, 2, 7, (40, 40)), (4, 4, 13, (64, 48))):
        images, context = torch.randn(te, 3, 224, 224, generator=g).to(cuda), torch.randn(te, 3, 336, 336, generator=g).to(cuda)
        sam = torch.randn(T, 3, 256, 256, generator=g).to(cuda)
        ids = torch.cat([torch.tensor([1, 5, 6]), torch.full((te,), -200), torch.randint(3, 4000, (n,), generator=g)])
        clips.append(([images], [context], [sam], ids[None], [(256, 256)], [hw]))
    m = VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.bfloat16, device=cuda)
    seg = cfg["seg_token_idx"]
    m.token_hook = lambda step, tok: seg if step in (2, 5) else None
    return m, clips


def _equal(got, ref):
    assert len(got) == len(ref)
    for b, ((o, s), (ro, rs)) in enumerate(zip(got, ref)):
        assert torch.equal(o, ro), b
        x, y = s[0], rs[0]
        assert len(s) == len(rs) == 1 and len(x) > 0
        assert sorted(x) == sorted(y) and all(sorted(x[t]) == sorted(y[t]) for t in x), b
        assert all(np.array_equal(x[t][k], y[t][k]) for t in x for k in x[t]), b


@pytest.mark.parametrize("video", [False, True])
def test_facade_equals_inference(cuda, video):
    """entry b of inference_clips() equals inference() on clip b — ids and masks pixel for pixel, in bf16 — greedy and sampled, and the
    group decoded on the batched state"""
    m, clips = _micro(cuda)
    kw = dict(max_new_tokens=10, use_sam2_video_branch=video)
    ref = [m.inference(*c, **kw) for c in clips]
    got = m.inference_clips(clips, **kw)
    _equal(got, ref)
    (key, rows), = m.P._decoder._rows.items()
    assert rows.row0 == 0 and rows.B == 4 and rows.steps == 9
    assert len({len(s[0]) for _, s in got}) == 3 and len({o.shape[1] for o, _ in got}) == 3      # other frame counts, other lengths
    # sampled: one seed per clip from the default generator, in list order
    sk = dict(kw, do_sample=True, top_k=20, top_p=0.9, temperature=0.8)
    torch.manual_seed(1234)
    ref_s = [m.inference(*c, **sk) for c in clips]
    torch.manual_seed(1234)
    got_s = m.inference_clips([dict(zip(("images", "context_images", "images_for_sam", "input_ids", "resize_list", "original_size_list"), c))
                               for c in clips], **sk)
    _equal(got_s, ref_s)
    assert rows.steps == 18 and rows.route == "sample_fast"
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(got_s, got))
