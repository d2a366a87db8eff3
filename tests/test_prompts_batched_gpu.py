"""The batched multi-prompt decode step on the HIP kernels: every B-row kernel gives each row the bits of its single-row counterpart,
and prompts.generate_prompts() on the batched step returns exactly what its sequential loop (VG_PROMPTS_BATCHED=0) returns."""
import functools

import numpy as np
import pytest
import torch

torch.set_grad_enabled(False)


class _Towers:
    def __init__(self, visual):
        self.visual = visual

    def encode(self, images, context_images, comm=None):
        return self.visual


@functools.lru_cache(maxsize=1)
def _weights():
    from oracle import seeded
    from videoglamm_amd import synth
    full = synth.videoglamm_llama3_8b()
    c = dict(full["llm"], num_layers=2, vocab=8192)
    man = {k: v for k, v in synth.vlm_manifest(dict(full, llm=c)).items()
           if k.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head", "model.text_hidden_fcs"))}
    return c, seeded.seeded_state_dict(man, 5)


def _llm(cuda, nvis=96):
    """2-layer synthetic Llama-3-8B-width LLM (bf16), visual block of nvis rows: the prefix is 3 text ids + nvis rows"""
    from videoglamm_amd.params import Params
    c, sd = _weights()
    sd = {k: (v.to(torch.bfloat16) if v.dim() >= 2 else v) for k, v in sd.items()}
    P = Params(sd, cuda, torch.bfloat16)
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


# ------------------------------------------------------------------ kernels, row by row against the single-row kernels
ROWS = [1, 2, 3, 5, 8, 16]


@pytest.mark.gpu
@pytest.mark.parametrize("B", ROWS)
def test_gemv_rows_bitwise(cuda, B):
    from videoglamm_amd import ops
    P, cfg, _ = _llm(cuda)
    c = cfg["llm"]
    l = "model.layers.0."
    g = torch.Generator().manual_seed(B)
    wgu, _ = P.fused([l + "mlp.gate_proj", l + "mlp.up_proj"], stored=l + "mlp.gate_up_proj")
    ffn = wgu.shape[0] // 2
    x = (torch.randn(B, c["hidden"], generator=g) * 2).to(torch.bfloat16).to(cuda)
    res = torch.randn(B, c["hidden"], generator=g).to(torch.bfloat16).to(cuda)
    a = (torch.randn(B, ffn, generator=g) * 0.3).to(torch.bfloat16).to(cuda)
    nw = P.f32(l + "post_attention_layernorm.weight")
    cases = [
        (x, P.w(l + "self_attn.o_proj"), dict(residual=res)),                                                   # o + residual
        (x, wgu, dict(norm_w=nw, eps=c["rms_eps"], glu=True)),                                                  # norm + gate|up + SwiGLU
        (a, P.w(l + "mlp.down_proj"), dict(residual=res)),                                                       # down (K = 14336: staged in phases)
        (x, P.w(l + "self_attn.o_proj"), dict(norm_w=nw, eps=c["rms_eps"])),                                     # norm, no epilogue
    ]
    for xin, w, kw in cases:
        got = ops.decode_gemv_rows(xin, w, **kw)
        for r in range(B):
            kr = dict(kw)
            if "residual" in kr:
                kr["residual"] = kr["residual"][r:r + 1].contiguous()
            want = ops.decode_gemv(xin[r:r + 1].contiguous(), w, **kr)
            assert torch.equal(got[r:r + 1], want), (w.shape, kw.keys(), r)


@pytest.mark.gpu
@pytest.mark.parametrize("B", ROWS)
def test_lm_head_rows_bitwise(cuda, B):
    """ops.linear runs the lm_head of <= 16 rows on the skinny GEMM: row r of a B-row call is the 1-row call's"""
    from videoglamm_amd import ops
    P, cfg, _ = _llm(cuda)
    h = torch.randn(B, cfg["llm"]["hidden"], generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).to(cuda)
    got = ops.linear(h, P.w("lm_head"), out_dtype=torch.float32)
    fin = ops.rmsnorm(h, P.f32("model.norm.weight"), cfg["llm"]["rms_eps"])
    for r in range(B):
        assert torch.equal(got[r:r + 1], ops.linear(h[r:r + 1], P.w("lm_head"), out_dtype=torch.float32))
        assert torch.equal(fin[r:r + 1], ops.rmsnorm(h[r:r + 1], P.f32("model.norm.weight"), cfg["llm"]["rms_eps"]))


def _decoder(P, cfg, max_len):
    from videoglamm_amd.vlm import LlamaDecoder
    dec = LlamaDecoder(P, cfg["llm"], max_len)
    assert dec.rope_path
    return dec


@pytest.mark.gpu
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("Ppre", [256, 255, 257, 99])
def test_qkv_rope_and_attention_rows_bitwise(cuda, B, Ppre):
    """q|k|v + RoPE + append and the attention per row, rows at distinct positions (suffixes of unequal length) in scattered slots, the prefix on,
    just before and just past a key-block boundary, against the single-row kernels on a whole cache holding the same rows"""
    from videoglamm_amd import ops
    from videoglamm_amd.prompts import slot_layout
    P, cfg, _ = _llm(cuda)
    c = cfg["llm"]
    dec = _decoder(P, cfg, 1024)
    H, Hkv, hd = dec.H, dec.Hkv, dec.hd
    g = torch.Generator().manual_seed(B * 1000 + Ppre)
    n_bound = Ppre + 80
    row0, _ = slot_layout(Ppre, dec.kpw2, n_bound)
    slots = 16
    perm = torch.randperm(slots, generator=g)[:B].tolist()          # row r lives in slot perm[r] of a 16-slot array
    pos = [Ppre + int(torch.randint(0, 60, (1,), generator=g)) for _ in range(B)]
    pref_k = (torch.randn(1024, Hkv, hd, generator=g)).to(torch.bfloat16).to(cuda)
    pref_v = (torch.randn(1024, Hkv, hd, generator=g)).to(torch.bfloat16).to(cuda)
    ks = (torch.randn(slots, n_bound - row0, Hkv, hd, generator=g)).to(torch.bfloat16).to(cuda)
    vs = (torch.randn(slots, n_bound - row0, Hkv, hd, generator=g)).to(torch.bfloat16).to(cuda)
    x = (torch.randn(B, c["hidden"], generator=g) * 2).to(torch.bfloat16).to(cuda)
    l = "model.layers.1."
    wqkv, _ = P.fused([l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj"], stored=l + "self_attn.qkv_proj")
    nw = P.f32(l + "input_layernorm.weight")
    # the rows kernels see slots perm[r] through views that start at slot perm[r]: use a gather into a B-slot array instead (row r = slot r),
    # keeping the scattered contents
    ksB, vsB = ks[perm].contiguous(), vs[perm].contiguous()
    pos_dev = torch.tensor(pos, dtype=torch.int32, device=cuda)
    rope_cs = torch.stack([torch.cat([dec.cos[p], dec.sin[p]]) for p in pos]).contiguous()
    q = ops.decode_qkv_rope_rows(x, wqkv, nw, c["rms_eps"], ksB, vsB, row0, rope_cs, pos_dev, H, Hkv, hd)
    ws = ops.decode_attention2_rows_workspace(H, Hkv, hd, n_bound, dec.kpw2, B, cuda)
    o = ops.decode_attention2_rows(q, pref_k, pref_v, ksB, vsB, row0, H, Hkv, hd, pos_dev, n_bound, hd ** -0.5, ws, keys_per_wg=dec.kpw2)
    o2 = ops.decode_attention2_rows(q, pref_k, pref_v, ksB, vsB, row0, H, Hkv, hd, pos_dev, n_bound, hd ** -0.5, ws, keys_per_wg=dec.kpw2)
    assert torch.equal(o, o2)                                   # the self-resetting counters
    ws1 = ops.decode_attention_workspace(H, Hkv, hd, 1024, cuda)
    for r in range(B):
        kc = pref_k.clone()
        vc = pref_v.clone()
        kc[row0:n_bound] = ks[perm[r]]
        vc[row0:n_bound] = vs[perm[r]]
        p1 = torch.tensor([pos[r]], dtype=torch.int32, device=cuda)
        q1 = ops.decode_qkv_rope(x[r:r + 1].contiguous(), wqkv, nw, c["rms_eps"], kc, vc, rope_cs[r].contiguous(), p1, H, Hkv, hd)
        assert torch.equal(q[r:r + 1], q1)
        assert torch.equal(ksB[r], kc[row0:n_bound]) and torch.equal(vsB[r], vc[row0:n_bound])      # the appended rows, and nothing else moved
        o1 = ops.decode_attention2(q1, kc, vc, H, Hkv, hd, p1, hd ** -0.5, ws1, keys_per_wg=dec.kpw2)
        assert torch.equal(o[r:r + 1], o1), r


@pytest.mark.gpu
@pytest.mark.parametrize("B", ROWS)
def test_step_head_tail_rows(cuda, B):
    """embed + cos / sin rows, and the tail: token from the accumulator, forcing, hist / raw, the final-norm row store, step and position bumps"""
    from videoglamm_amd import ops
    P, cfg, _ = _llm(cuda)
    dec = _decoder(P, cfg, 1024)
    g = torch.Generator().manual_seed(B)
    table = P.t("model.embed_tokens.weight")
    tok = torch.randint(0, 8192, (B,), generator=g).to(cuda)
    pos = torch.randint(200, 900, (B,), generator=g).to(torch.int32).to(cuda)      # past every hid_row0 below
    rope_cs = torch.zeros(B, dec.hd, device=cuda)
    x = ops.decode_step_begin_rows(tok, table, pos, rope=(dec.cos, dec.sin, rope_cs))
    for r in range(B):
        cs = torch.zeros(dec.hd, device=cuda)
        x1 = ops.decode_step_begin(tok[r:r + 1], table, pos[r:r + 1], rope=(dec.cos, dec.sin, cs))
        assert torch.equal(x[r:r + 1], x1) and torch.equal(rope_cs[r], cs)
    logits = torch.randn(B, 8192, generator=g).to(cuda)
    acc = torch.zeros(B, dtype=torch.int64, device=cuda)
    ops.argmax_partial_rows(logits, acc)
    step = torch.randint(0, 6, (B,), generator=g).to(torch.int32).to(cuda)
    forced = torch.full((B, 8), -1, dtype=torch.int64)
    for r in range(0, B, 2):
        forced[r, int(step[r])] = 4242 + r                          # every other row is forced at its step
    forced = forced.to(cuda)
    hist = torch.zeros(B, 8, dtype=torch.int64, device=cuda)
    raw = torch.zeros_like(hist)
    hid = torch.zeros(B, 1024, dec.D, dtype=torch.bfloat16, device=cuda)
    rows = torch.randn(B, dec.D, generator=g).to(torch.bfloat16).to(cuda)
    pos0, step0 = pos.clone(), step.clone()
    tok2 = tok.clone()
    hid_row0 = 64 * (B % 3)                                         # slots that start past row 0 (RowsDecode: at row0)
    hidw = torch.zeros(B, 1024 - hid_row0, dec.D, dtype=torch.bfloat16, device=cuda)
    ops.decode_step_end_rows(acc, tok2, pos, step, rows, hidw, forced=forced, hist=hist, raw=raw, hid_row0=hid_row0)
    hid[:, hid_row0:] = hidw
    assert int(acc.abs().sum()) == 0
    for r in range(B):
        a1 = torch.zeros(1, dtype=torch.int64, device=cuda)
        ops.argmax_partial(logits[r], a1)
        t1, p1, s1 = tok[r:r + 1].clone(), pos0[r:r + 1].clone(), step0[r:r + 1].clone()
        h1 = torch.zeros(1024, dec.D, dtype=torch.bfloat16, device=cuda)
        hi1, ra1 = torch.zeros(8, dtype=torch.int64, device=cuda), torch.zeros(8, dtype=torch.int64, device=cuda)
        ops.decode_step_end(a1, t1, p1, s1, rows[r:r + 1], h1, forced=forced[r].contiguous(), hist=hi1, raw=ra1)
        assert int(t1) == int(tok2[r]) and int(p1) == int(pos[r]) == int(pos0[r]) + 1 and int(s1) == int(step[r]) == int(step0[r]) + 1
        assert torch.equal(hi1, hist[r]) and torch.equal(ra1, raw[r]) and torch.equal(h1, hid[r])
        assert int(raw[r, int(step0[r])]) == int(logits[r].argmax())
        if r % 2 == 0:
            assert int(tok2[r]) == 4242 + r


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


@pytest.mark.gpu
def test_seventeen_prompts_in_groups_of_sixteen(cuda, monkeypatch):
    """17 = 16 + 1 as model.inference_prompts groups them: the 16-prompt group runs the batched step (16 rows, as many steps as its longest prompt),
    the last prompt the single-row loop; together they equal the sequential loop over all 17"""
    P, cfg, tw = _llm(cuda)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step in (1, 4) else None
    ids = _prompts(17, 6)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = _run(P, cfg, tw, ids, 8, hook=hook)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    P._decoder._rows = {}
    a = _run(P, cfg, tw, ids[:16], 8, hook=hook)
    rows = next(iter(P._decoder._rows.values()))
    assert rows.B == 16 and rows.steps == 7
    b = _run(P, cfg, tw, ids[16:], 8, hook=hook)
    _same(ref, (a[0] + b[0], a[1] + b[1]))


@pytest.mark.gpu
def test_step_past_the_slots_is_refused(cuda, monkeypatch):
    P, cfg, tw = _llm(cuda)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    _run(P, cfg, tw, _prompts(3), 4)
    rows = next(iter(P._decoder._rows.values()))
    with pytest.raises(AssertionError):
        rows.set_positions([rows.n_bound] * rows.B)
    rows.host_pos = [rows.n_bound] * rows.B
    with pytest.raises(ValueError):
        rows.decode_step()


@pytest.mark.gpu
@pytest.mark.parametrize("nvis", [252, 253, 254])
def test_prefix_at_a_key_block_boundary(cuda, monkeypatch, nvis):
    """P = 255, 256, 257: the prefix ends just before, on and just past a 256-key block"""
    P, cfg, tw = _llm(cuda, nvis)
    ref, got = _both(monkeypatch, P, cfg, tw, _prompts(5, 1), 10)
    _same(ref, got)


@pytest.mark.gpu
def test_eos_at_different_steps(cuda, monkeypatch):
    P, cfg, tw = _llm(cuda)
    ids = _prompts(6, 2)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    free, _ = _run(P, cfg, tw, ids, 12)
    # every prompt's own token at steps 2..7 as its EOS: the prompts stop at different steps
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
    # a new seed is a copy into the parameter block: the captured step draws other tokens
    sp2 = [dict(s, seed=s["seed"] + 7) for s in sp]
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref2 = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp2)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got2 = _run(P, cfg, tw, _prompts(B, 3), 8, samplings=sp2)
    _same(ref2, got2)


@pytest.mark.gpu
def test_graph_replay_equals_eager(cuda, monkeypatch):
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, tw = _llm(cuda)
    seg = cfg["seg_token_idx"]
    hook = lambda step, tok: seg if step == 3 else None
    ids = _prompts(5, 4)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    a = _run(P, cfg, tw, ids, 8, hook=hook)
    P._decoder = LlamaDecoder(P, cfg["llm"], 1024, use_graph=False)
    b = _run(P, cfg, tw, ids, 8, hook=hook)
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
    rows = next(iter(P._decoder._rows.values()))
    gen = [len(o) - len(x) for o, x in zip(got, ids)]
    assert rows.B == 8 and rows.steps == max(gen) - 1 and rows.steps < sum(gen) - len(gen)
