"""model.inference_prompts() / prompts.generate_prompts() on the HIP kernels: each prompt gives what inference() / generate()
give for it alone, and a prompt's ids and [SEG] embeddings do not depend on the prompts it is batched with."""
import functools

import numpy as np
import pytest
import torch

torch.set_grad_enabled(False)

V = 96          # visual rows of the synthetic clips (the prefix is 3 text ids + the visual block)


class _Towers:
    """towers.encode stand-in: the LLM-side tests hand the decoder a fixed visual block"""

    def __init__(self, visual):
        self.visual = visual

    def encode(self, images, context_images, comm=None):
        return self.visual


@functools.lru_cache(maxsize=2)
def _weights(kind):
    from oracle import seeded
    from videoglamm_amd import synth
    full = synth.videoglamm_llama3_8b() if kind == "llama" else synth.videoglamm_phi3_mini()
    c = dict(full["llm"], num_layers=2, vocab=8192)
    if kind == "phi3":
        c["sliding_window"] = 63
    man = {k: v for k, v in synth.vlm_manifest(dict(full, llm=c)).items()
           if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head", "model.text_hidden_fcs"))}
    return c, seeded.seeded_state_dict(man, 5)


def _llm(cuda, kind, dtype):
    """2-layer synthetic LLMs: Llama-3-8B width (head_dim 128, G = 4) or Phi-3-mini width (head_dim 96, MHA, fused projections, a window
    shorter than the prefix)"""
    from videoglamm_amd.params import Params
    c, sd = _weights(kind)
    sd = {k: (v.to(dtype) if v.dim() >= 2 else v) for k, v in sd.items()}
    P = Params(sd, cuda, dtype)
    visual = (torch.randn(V, c["hidden"], generator=torch.Generator().manual_seed(3)) * 0.5).to(dtype).to(cuda)
    return P, dict(llm=c, seg_token_idx=8191), _Towers(visual)


def _prompts(n, seed=0):
    """n prompts with one prefix [1, 5, 6, <image> x 4] and questions of 0..9 ids"""
    g = torch.Generator().manual_seed(seed)
    head = torch.tensor([1, 5, 6, -200, -200, -200, -200])
    return [torch.cat([head, torch.randint(10, 8000, ((3 * b + 4) % 10,), generator=g)]) for b in range(n)]


def _alone(P, cfg, tw, ids, n, eos=None, hook=None, sampling=None):
    from videoglamm_amd import vlm
    out, emb = vlm.generate(P, cfg, None, None, None, ids, n, eos, visual=tw.visual, token_hook=hook, sampling=sampling)
    return out.tolist(), emb


def _batch(P, cfg, tw, ids_list, n, eos=None, hook=None, samplings=None):
    from videoglamm_amd.prompts import generate_prompts
    out, emb, counts = generate_prompts(P, cfg, tw, None, None, ids_list, n, eos, token_hook=hook, samplings=samplings)
    starts = np.cumsum([0] + counts)
    return [o.tolist() for o in out], [emb[a:b] for a, b in zip(starts[:-1], starts[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["llama", "phi3"])
def test_llm_parity_fp32(cuda, kind):
    """each prompt's ids equal generate()'s for it alone; [SEG] embeddings within 1e-3.  Every [SEG] comes from the token hook at steps 1
    and 4, so the rows are taken from the suffix's prefill and from decode steps."""
    P, cfg, tw = _llm(cuda, kind, torch.float32)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None
    ids = _prompts(4)
    n = 8
    got, embs = _batch(P, cfg, tw, ids, n, hook=hook)
    for b, x in enumerate(ids):
        want, emb = _alone(P, cfg, tw, x, n, hook=hook)
        assert got[b] == want, b
        assert embs[b].shape == emb.shape == (2, 256)
        torch.testing.assert_close(embs[b], emb, rtol=1e-3, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("sampled", [False, True])
def test_batch_invariance(cuda, dtype, sampled):
    """a prompt alone and in a batch of 5, in two orders: bit-identical ids and [SEG] embeddings (sampling: the same seed for the prompt)"""
    P, cfg, tw = _llm(cuda, "llama", dtype)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (0, 3) else None
    ids = _prompts(5, seed=1)
    samp = [dict(T=1.5, k=0, p=0.95, seed=100 + b) for b in range(5)] if sampled else None
    n = 7
    alone = [_batch(P, cfg, tw, [ids[b]], n, hook=hook, samplings=None if samp is None else [samp[b]]) for b in range(5)]
    fwd = _batch(P, cfg, tw, ids, n, hook=hook, samplings=samp)
    order = [3, 0, 4, 2, 1]
    rev = _batch(P, cfg, tw, [ids[b] for b in order], n, hook=hook, samplings=None if samp is None else [samp[b] for b in order])
    for b in range(5):
        (a_ids,), (a_emb,) = alone[b]
        r = order.index(b)
        assert fwd[0][b] == a_ids and rev[0][r] == a_ids
        assert torch.equal(fwd[1][b], a_emb) and torch.equal(rev[1][r], a_emb)


@pytest.mark.gpu
def test_stopping_and_forcing(cuda, monkeypatch):
    """EOS at different steps for different prompts, max_new_tokens, and a forced-token table (applied on the device under VG_DECODE_AHEAD=1):
    every prompt of the batch stops and is forced as it is when it runs alone (bf16: the reference is the prompt alone through the same path)"""
    from videoglamm_amd import synth
    P, cfg, tw = _llm(cuda, "llama", torch.bfloat16)
    ids = _prompts(4, seed=2)
    n = 10
    alone = lambda x, **k: [v[0] for v in _batch(P, cfg, tw, [x], n, **k)]
    free = [alone(x)[0] for x in ids]
    assert all(len(f) == len(x) + n for f, x in zip(free, ids))          # max_new_tokens
    # an EOS set with one id of each prompt's output at a different step: every prompt stops at its own first EOS id
    eos = {free[b][len(ids[b]) + 2 * b] for b in range(3)}
    got, _ = _batch(P, cfg, tw, ids, n, eos=eos)
    for b, x in enumerate(ids):
        want = alone(x, eos=eos)[0]
        assert got[b] == want and (len(want) == len(x) + n or want[-1] in eos)
        stop = [j for j in range(len(x), len(free[b])) if free[b][j] in eos]
        assert want == free[b][:stop[0] + 1] if stop else want == free[b]
    assert len({len(g) - len(x) for g, x in zip(got, ids)}) > 1          # they did stop at different steps
    table = {1: cfg["seg_token_idx"], 2: 77, 5: cfg["seg_token_idx"]}
    hook = synth.forced_tokens_hook(table)
    for ahead in ("0", "1"):
        monkeypatch.setenv("VG_DECODE_AHEAD", ahead)
        got, embs = _batch(P, cfg, tw, ids, n, hook=hook)
        for b, x in enumerate(ids):
            want, emb = alone(x, hook=hook)
            assert got[b] == want and all(got[b][len(x) + j] == t for j, t in table.items())
            assert embs[b].shape[0] == 2 and torch.equal(embs[b], emb)


@pytest.mark.gpu
def test_graph_replay_matches_eager(cuda):
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, tw = _llm(cuda, "phi3", torch.bfloat16)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step == 2 else None
    ids = _prompts(3, seed=4)
    graphed = _batch(P, cfg, tw, ids, 6, hook=hook)
    P._decoder = LlamaDecoder(P, cfg["llm"], P._decoder.max_len, use_graph=False)
    eager = _batch(P, cfg, tw, ids, 6, hook=hook)
    assert graphed[0] == eager[0] and all(torch.equal(a, b) for a, b in zip(graphed[1], eager[1]))


def _tiny(cuda):
    from test_oracle_e2e import e2e_setup
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    fx, sd, cfg, inp = e2e_setup()
    m = VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.float32, device=cuda)
    base = inp["input_ids"]
    n0 = int((base == -200).nonzero().max()) + 1
    ids = [base, torch.cat([base[:n0], torch.tensor([84, 12, 99, 150, 7])]), base[:n0]]
    return m, inp, ids


@pytest.mark.gpu
@pytest.mark.parametrize("video", [False, True])
def test_tiny_model_parity(cuda, video):
    """the tiny e2e model in fp32, both SAM2 branches: ids and masks equal inference()'s per prompt, [SEG] embeddings and mask logits within
    1e-3; objects of several prompts share one SAM2 call"""
    m, inp, ids = _tiny(cuda)
    seg = m.config.seg_token_idx
    m.token_hook = lambda step, tok: seg if step == 1 else None
    clip = ([inp["images"]], [inp["context_images"]], [inp["images_for_sam"]])
    rest = ([(1024, 1024)], [inp["original_size"]])
    ref = []
    for x in ids:
        m.capture = {}
        o, s = m.inference(*clip, x[None], *rest, max_new_tokens=3, use_sam2_video_branch=video)
        ref.append((o, s[0], m.capture))
    m.capture = {}
    out, segs = m.inference_prompts(*clip, ids, *rest, max_new_tokens=3, use_sam2_video_branch=video)
    cap = m.capture
    m.capture = None
    fast = m.inference_prompts(*clip, ids, *rest, max_new_tokens=3, use_sam2_video_branch=video)
    for b, (o, s, c) in enumerate(ref):
        assert torch.equal(out[b], o) and torch.equal(fast[0][b], o)
        torch.testing.assert_close(cap["emb"][b], c["emb"], rtol=1e-3, atol=1e-3)
        torch.testing.assert_close(cap["logits"][b], c["logits"], rtol=1e-3, atol=1e-3)
        for got in (segs[b], fast[1][b]):
            assert sorted(got) == sorted(s)
            m_got = np.stack([np.stack([got[t][k] for k in sorted(got[t])]) for t in sorted(got)])
            m_ref = np.stack([np.stack([s[t][k] for k in sorted(s[t])]) for t in sorted(s)])
            assert m_got.shape == m_ref.shape and (m_got & m_ref).sum() / max((m_got | m_ref).sum(), 1) > 0.999


@pytest.mark.gpu
def test_sampling_seeds_in_list_order(cuda):
    """sampling: one seed per prompt drawn from the generator in list order — the same ids as inference() per prompt in that order"""
    m, inp, ids = _tiny(cuda)
    clip = ([inp["images"]], [inp["context_images"]], [inp["images_for_sam"]])
    rest = ([(1024, 1024)], [inp["original_size"]])
    kw = dict(max_new_tokens=5, use_sam2_video_branch=True, do_sample=True, temperature=3.0)
    torch.manual_seed(11)
    want = [m.inference(*clip, x[None], *rest, **kw)[0] for x in ids]
    torch.manual_seed(11)
    got = m.inference_prompts(*clip, ids, *rest, **kw)[0]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    g = torch.Generator().manual_seed(11)
    assert all(torch.equal(a, b) for a, b in zip(m.inference_prompts(*clip, ids, *rest, generator=g, **kw)[0], want))
