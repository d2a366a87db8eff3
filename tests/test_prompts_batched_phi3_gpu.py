"""The batched multi-prompt decode step of the decode_attention path (Phi-3-mini width) on the HIP kernels: the B-row GEMVs at
K = 3072 and vg_decode_attention_rows give each row the bits of the single-row kernels, and prompts.generate_prompts() on the batched step returns
exactly what its sequential loop (VG_PROMPTS_BATCHED=0) returns."""
import functools

import numpy as np
import pytest
import torch

torch.set_grad_enabled(False)

NVIS = 297          # prefix = 3 text ids + the visual block: P = 300 (row0 = 256: two shared 128-key blocks)


class _Towers:
    def __init__(self, visual):
        self.visual = visual

    def encode(self, images, context_images, comm=None):
        return self.visual


@functools.lru_cache(maxsize=1)
def _weights():
    from oracle import seeded
    from videoglamm_amd import synth
    full = synth.videoglamm_phi3_mini()
    c = dict(full["llm"], num_layers=2, vocab=8192)
    man = {k: v for k, v in synth.vlm_manifest(dict(full, llm=c)).items()
           if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head", "model.text_hidden_fcs"))}
    sd = seeded.seeded_state_dict(man, 5)
    return c, {k: (v.to(torch.bfloat16) if v.dim() >= 2 else v) for k, v in sd.items()}


def _llm(cuda, nvis=NVIS, window=199):
    """2-layer synthetic Phi-3-mini-width LLM (bf16: hidden 3072, 32 MHA heads of 96, ffn 8192), sliding window `window` (attends window + 1
    keys), visual block of nvis rows"""
    from videoglamm_amd.params import Params
    c, sd = _weights()
    c = dict(c, sliding_window=window)
    P = Params(dict(sd), cuda, torch.bfloat16)
    visual = (torch.randn(nvis, c["hidden"], generator=torch.Generator().manual_seed(3)) * 0.5).to(torch.bfloat16).to(cuda)
    return P, dict(llm=c, seg_token_idx=8191), _Towers(visual)


def _prompts(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    head = torch.tensor([1, 5, 6, -200, -200, -200, -200])
    return [torch.cat([head, torch.randint(10, 8000, ((3 * b + 4) % 10,), generator=g)]) for b in range(n)]


def _run(P, cfg, tw, ids, n, eos=None, hook=None, samplings=None, traces=None):
    from videoglamm_amd.prompts import generate_prompts
    out, emb, counts = generate_prompts(P, cfg, tw, None, None, ids, n, eos, token_hook=hook, samplings=samplings, traces=traces)
    starts = np.cumsum([0] + counts)
    return [o.tolist() for o in out], [emb[a:b].cpu() for a, b in zip(starts[:-1], starts[1:])]


def _both(monkeypatch, P, cfg, tw, ids, n, **kw):
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, ids, n, **kw)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got = _run(P, cfg, tw, ids, n, **kw)
    return ref, got


def _same(ref, got):
    assert got[0] == ref[0]
    assert len(got[1]) == len(ref[1])
    for a, b in zip(got[1], ref[1]):
        assert torch.equal(a, b)


def _rows(P):
    rows = next(iter(P._decoder._rows.values()))
    assert rows.attn_rows
    return rows


# ------------------------------------------------------------------ kernels, row by row against the single-row kernels
ROWS = [1, 2, 5, 8, 16]


@pytest.mark.gpu
def test_step_is_covered(cuda):
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = _llm(cuda)
    dec = LlamaDecoder(P, cfg["llm"], 1024)
    assert not dec.rope_path and dec.fused_decode and (dec.H, dec.Hkv, dec.hd, dec.D) == (32, 32, 96, 3072)
    assert ops.decode_step_rows_supported(dec.H, dec.Hkv, dec.hd, dec.D, 8192, torch.bfloat16)
    assert not ops.decode_step_rows_supported(dec.H, dec.Hkv, dec.hd, dec.D, 8192, torch.float32)
    assert not ops.decode_step_rows_supported(32, 8, 128, 4096, 14336, torch.bfloat16)          # Llama-3: the rope path's kernels
    assert not ops.decode_rows_supported(dec.H, dec.Hkv, dec.hd, dec.D, 8192, torch.bfloat16)    # unchanged: Llama widths only


@pytest.mark.gpu
@pytest.mark.parametrize("B", ROWS)
def test_gemv_rows_k3072_bitwise(cuda, B):
    from videoglamm_amd import ops
    P, cfg, _ = _llm(cuda)
    c = cfg["llm"]
    l = "model.layers.0."
    g = torch.Generator().manual_seed(B)
    wqkv, _ = P.fused([l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj"], stored=l + "self_attn.qkv_proj")
    wgu, _ = P.fused([l + "mlp.gate_proj", l + "mlp.up_proj"], stored=l + "mlp.gate_up_proj")
    assert wqkv.shape == (9216, 3072) and wgu.shape == (16384, 3072)
    x = (torch.randn(B, 3072, generator=g) * 2).to(torch.bfloat16).to(cuda)
    res = torch.randn(B, 3072, generator=g).to(torch.bfloat16).to(cuda)
    a = (torch.randn(B, 8192, generator=g) * 0.3).to(torch.bfloat16).to(cuda)
    cases = [
        (x, wqkv, dict(norm_w=P.f32(l + "input_layernorm.weight"), eps=c["rms_eps"])),                          # norm + q|k|v (N = 9216)
        (x, P.w(l + "self_attn.o_proj"), dict(residual=res)),                                                   # o + residual (staged in phases at 16 rows)
        (x, wgu, dict(norm_w=P.f32(l + "post_attention_layernorm.weight"), eps=c["rms_eps"], glu=True)),        # norm + gate|up + SwiGLU
        (a, P.w(l + "mlp.down_proj"), dict(residual=res)),                                                       # down (K = 8192)
    ]
    for xin, w, kw in cases:
        got = ops.decode_gemv_rows(xin, w, **kw)
        for r in range(B):
            kr = dict(kw)
            if "residual" in kr:
                kr["residual"] = kr["residual"][r:r + 1].contiguous()
            want = ops.decode_gemv(xin[r:r + 1].contiguous(), w, **kr)
            assert torch.equal(got[r:r + 1], want), (w.shape, sorted(kw), r)


@pytest.mark.gpu
@pytest.mark.parametrize("B", ROWS)
def test_lm_head_rows_bitwise(cuda, B):
    """the lm_head at the released width (K = 3072, N = 32065): row r of the B-row ops.linear is the 1-row call's"""
    from videoglamm_amd import ops
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(32065, 3072, generator=g) * 0.02).to(torch.bfloat16).to(cuda)
    h = torch.randn(B, 3072, generator=g).to(torch.bfloat16).to(cuda)
    got = ops.linear(h, w, out_dtype=torch.float32)
    for r in range(B):
        assert torch.equal(got[r:r + 1], ops.linear(h[r:r + 1], w, out_dtype=torch.float32)), r


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 16])
@pytest.mark.parametrize("kpw", ["split", "64", "128"])
@pytest.mark.parametrize("window", [63, 200])
@pytest.mark.parametrize("Ppre", [300, 520, 512])
def test_attention_rows_bitwise(cuda, B, kpw, window, Ppre):
    """RoPE + append + attention per row, rows at distinct positions in their own slots, the prefix inside a 128-key block (300, 520) and on its
    boundary (512), the window's first key in the shared blocks or in the slot, and rows of one launch on 64- and 128-key splits, against
    vg_decode_attention on a whole cache holding the same rows"""
    from videoglamm_amd import ops
    from videoglamm_amd.prompts import slot_layout
    from videoglamm_amd.vlm import LlamaDecoder, RowsDecode
    P, cfg, _ = _llm(cuda)
    dec = LlamaDecoder(P, cfg["llm"], 1024)
    H, Hkv, hd = dec.H, dec.Hkv, dec.hd
    g = torch.Generator().manual_seed(B * 1000 + Ppre + window)
    n_bound = Ppre + 80
    row0, _ = slot_layout(Ppre, RowsDecode.ATTN_KW, n_bound)
    pos = [Ppre + int(torch.randint(0, 80, (1,), generator=g)) for _ in range(B)]
    pos[0] = Ppre                                               # the first decode row of a prompt without a suffix
    kpw_min = {"split": sorted(pos)[B // 2], "64": 8192, "128": 0}[kpw]
    pref_k = torch.randn(1024, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    pref_v = torch.randn(1024, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    ks = torch.randn(B, n_bound - row0, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    vs = torch.randn(B, n_bound - row0, Hkv, hd, generator=g).to(torch.bfloat16).to(cuda)
    ks0, vs0, pk0, pv0 = ks.clone(), vs.clone(), pref_k.clone(), pref_v.clone()
    qkv = torch.randn(B, (H + 2 * Hkv) * hd, generator=g).to(torch.bfloat16).to(cuda)
    pos_dev = torch.tensor(pos, dtype=torch.int32, device=cuda)
    ws = ops.decode_attention_rows_workspace(H, Hkv, hd, n_bound, B, cuda)
    args = (qkv, pref_k, pref_v, ks, vs, row0, dec.cos, dec.sin, H, Hkv, hd, pos_dev, n_bound, hd ** -0.5, ws)
    o = ops.decode_attention_rows(*args, window=window, kpw_min=kpw_min)
    o2 = ops.decode_attention_rows(*args, window=window, kpw_min=kpw_min)
    assert torch.equal(o, o2)                                   # the self-resetting counters (the second launch re-appends the same rows)
    assert torch.equal(pref_k, pk0) and torch.equal(pref_v, pv0)  # the shared prefix is read only
    ws1 = ops.decode_attention_workspace(H, Hkv, hd, 1024, cuda)
    for r in range(B):
        kc, vc = pk0.clone(), pv0.clone()
        kc[row0:n_bound] = ks0[r]
        vc[row0:n_bound] = vs0[r]
        p1 = torch.tensor([pos[r]], dtype=torch.int32, device=cuda)
        o1 = ops.decode_attention(qkv[r:r + 1].contiguous(), kc, vc, dec.cos, dec.sin, H, Hkv, hd, p1, hd ** -0.5, ws1, window=window,
                                  keys_per_wg=128 if pos[r] >= kpw_min else 0)
        assert torch.equal(o[r:r + 1], o1), r
        assert torch.equal(ks[r], kc[row0:n_bound]) and torch.equal(vs[r], vc[row0:n_bound]), r      # the appended rows, and nothing else moved


# ------------------------------------------------------------------ end to end: the batched route against VG_PROMPTS_BATCHED=0
@pytest.mark.gpu
@pytest.mark.parametrize("B", [2, 5, 16])
def test_greedy_batched_equals_sequential(cuda, monkeypatch, B):
    P, cfg, tw = _llm(cuda)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None        # [SEG] from the suffix prefill's row and from decode rows
    ref, got = _both(monkeypatch, P, cfg, tw, _prompts(B), 8, hook=hook)
    _same(ref, got)
    assert all(len(e) == 2 for e in got[1])
    assert _rows(P).B == (2 if B == 2 else 8 if B == 5 else 16)


@pytest.mark.gpu
@pytest.mark.parametrize("nvis,window", [(517, 62), (509, 199), (297, 62)])
def test_prefix_and_window_edges(cuda, monkeypatch, nvis, window):
    """P = 520 (row0 = 512) and P = 512 (on a 128-key boundary: row0 = P); windows of 63 and 200 keys whose first key falls in the shared blocks
    or in the slots"""
    P, cfg, tw = _llm(cuda, nvis, window)
    ref, got = _both(monkeypatch, P, cfg, tw, _prompts(5, 1), 10)
    _same(ref, got)
    rows = _rows(P)
    assert rows.row0 == (nvis + 3) // 128 * 128


@pytest.mark.gpu
def test_seventeen_prompts_in_groups_of_sixteen(cuda, monkeypatch):
    P, cfg, tw = _llm(cuda)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None
    ids = _prompts(17, 6)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, ids, 8, hook=hook)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    P._decoder._rows = {}
    a = _run(P, cfg, tw, ids[:16], 8, hook=hook)
    rows = _rows(P)
    assert rows.B == 16 and rows.steps == 7
    b = _run(P, cfg, tw, ids[16:], 8, hook=hook)
    _same(ref, (a[0] + b[0], a[1] + b[1]))


@pytest.mark.gpu
def test_eos_at_different_steps(cuda, monkeypatch):
    P, cfg, tw = _llm(cuda)
    ids = _prompts(6, 2)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    free, _ = _run(P, cfg, tw, ids, 12)
    eos = sorted({o[len(x) + 1 + b % 6] for b, (o, x) in enumerate(zip(free, ids))})
    ref, got = _both(monkeypatch, P, cfg, tw, ids, 12, eos=eos)
    _same(ref, got)
    assert len({len(o) - len(x) for o, x in zip(got[0], ids)}) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", [20, 0])          # fast route (1 <= k <= 64) / general route
@pytest.mark.parametrize("B", [2, 5, 16])
def test_sampled_batched_equals_sequential(cuda, monkeypatch, B, k):
    P, cfg, tw = _llm(cuda)
    sp = [dict(T=0.8, k=k, p=0.9, seed=100 + b) for b in range(B)]
    traces_a, traces_b = [{} for _ in range(B)], [{} for _ in range(B)]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp, traces=traces_a)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp, traces=traces_b)
    _same(ref, got)
    assert traces_a == traces_b
    assert _rows(P).route == ("sample_fast" if k else "sample")


@pytest.mark.gpu
def test_rows_cross_the_split_threshold_mid_decode(cuda, monkeypatch):
    """VG_DEC_KPW_MIN inside the decoded span (read when the decoder is built): rows move from 64- to 128-key splits at different steps within
    one captured graph, as the sequential loop moves from one captured graph to the other"""
    monkeypatch.setenv("VG_DEC_KPW_MIN", "310")
    P, cfg, tw = _llm(cuda)
    ids = _prompts(5, 7)
    ref, got = _both(monkeypatch, P, cfg, tw, ids, 14)
    _same(ref, got)
    rows = _rows(P)
    assert P._decoder.kpw_min == 310
    assert min(rows.start_pos) < 310 < max(rows.host_pos) and len(rows.graphs) == 1


@pytest.mark.gpu
def test_graph_replay_equals_eager(cuda, monkeypatch):
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, tw = _llm(cuda)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step == 3 else None
    ids = _prompts(5, 4)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    a = _run(P, cfg, tw, ids, 8, hook=hook)
    assert _rows(P).graphs
    P._decoder = LlamaDecoder(P, cfg["llm"], 1024, use_graph=False)
    b = _run(P, cfg, tw, ids, 8, hook=hook)
    assert not _rows(P).graphs
    _same(a, b)


@pytest.mark.gpu
def test_batched_route_is_taken(cuda, monkeypatch):
    """at B = 8 the batched step runs as many steps as the longest prompt decodes, not their sum"""
    P, cfg, tw = _llm(cuda)
    ids = _prompts(8, 5)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    free, _ = _run(P, cfg, tw, ids, 10)
    eos = [free[0][len(ids[0]) + 3]]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got, _ = _run(P, cfg, tw, ids, 10, eos=eos)
    rows = _rows(P)
    gen = [len(o) - len(x) for o, x in zip(got, ids)]
    assert rows.B == 8 and rows.steps == max(gen) - 1 and rows.steps < sum(gen) - len(gen)
