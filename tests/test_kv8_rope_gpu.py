"""The fp8 K/V cache on the rope decode step (cfg["llm"]["kv_cache"] = "fp8_rope") on the HIP kernels.  e4m3 -> bf16 is exact and the
kernels keep the bf16 kernels' order of every sum, so every comparison here is torch.equal: vg_decode_attention2_kv8 against vg_decode_attention2
on the dequantised cache (whose dropped / leaked / mis-weighted-key probes test_attention_accuracy_gpu.py holds), vg_decode_qkv_rope_kv8 against
the format's torch statement on the bf16 entry point's rows, the rows forms against the single-row forms, the decoder against a bf16-K/V decoder on
the rope step whose cache rows are rounded to e4m3 behind its back, and the batched entry points against their sequential loops."""
import functools

import numpy as np
import pytest
import torch

import test_prompts_batched_gpu as llama

torch.set_grad_enabled(False)

pytestmark = pytest.mark.gpu

D = 128
KMAX, VMIN = 0x7E, 0xFE          # +448 / -448: finite and huge — what a masked row holds here (the kernel masks, it does not skip: no NaN codes)
NAN8 = 0x7F


def _ref(x):
    """the format, as DESIGN 8c states it"""
    return x.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _deq(q):
    return q.view(torch.float8_e4m3fn).to(torch.bfloat16)


def _codes(shape, g, cuda, std=1.0):
    return _ref((torch.randn(*shape, generator=g) * std).to(torch.bfloat16)).to(cuda)


def _counters(ws, n):
    return int(ws[ws.numel() - n:].view(torch.int32).abs().sum())


# ------------------------------------------------------------------ 1. the attention against the bf16 kernel on the dequantised cache
HEADS = [(32, 8), (8, 8), (16, 8), (16, 2)]
POSITIONS = [0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000, 2047]


def _attention_case(cuda, H, Hkv, kpw, window, max_len, positions, g, k8m, v8m, qstd=1.0):
    """both kernels at every position on one workspace; rows past the position hold +-448"""
    from videoglamm_amd import ops
    ws = ops.decode_attention2_rows_workspace(H, Hkv, D, max_len, 128, 1, cuda)        # (one row: vg_decode_attention2's layout, at its finest split)
    for pos in positions:
        q = (torch.randn(1, H * D, generator=g) * qstd).to(torch.bfloat16).to(cuda)
        k8, v8 = k8m.clone(), v8m.clone()
        k8[pos + 1:], v8[pos + 1:] = KMAX, VMIN
        k8_0, v8_0 = k8.clone(), v8.clone()
        p = torch.tensor([pos], dtype=torch.int32, device=cuda)
        got = ops.decode_attention2_kv8(q, k8, v8, H, Hkv, D, p, D ** -0.5, ws, window=window, keys_per_wg=kpw)
        want = ops.decode_attention2(q, _deq(k8), _deq(v8), H, Hkv, D, p, D ** -0.5, ws, window=window, keys_per_wg=kpw)
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, want), (pos, kpw, window)
        assert torch.equal(k8, k8_0) and torch.equal(v8, v8_0), pos                      # the caches are read only
        yield pos, q, k8, v8, got
    assert _counters(ws, Hkv) == 0


@pytest.mark.parametrize("window", [0, 300])
@pytest.mark.parametrize("kpw", [128, 256])
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"{h[0]}x{h[1]}")
def test_attention_equals_bf16_kernel_on_dequantised_cache(cuda, heads, kpw, window):
    from videoglamm_amd import ops
    H, Hkv = heads
    assert ops.decode_rope_path_kv8(H, Hkv, D, 4096, torch.bfloat16) and not ops.decode_rope_path_kv8(H, Hkv, D, 4096, torch.float32)
    g = torch.Generator().manual_seed(H * 100 + Hkv + kpw + window)
    max_len = 2048
    k8m, v8m = _codes((max_len, Hkv, D), g, cuda), _codes((max_len, Hkv, D), g, cuda)
    outs = [o for *_, o in _attention_case(cuda, H, Hkv, kpw, window, max_len, POSITIONS, g, k8m, v8m)]
    assert len(outs) == len(POSITIONS)


@pytest.mark.parametrize("kpw,max_len,pos", [(128, 2304, 2200), (256, 8448, 8300)], ids=["18-splits-of-128", "33-splits-of-256"])
def test_attention_second_merge_pass(cuda, kpw, max_len, pos):
    """more partials than one merge pass takes (16 at 128 keys per workgroup, 32 at 256)"""
    H, Hkv = 32, 8
    assert pos // kpw + 1 > (16 if kpw == 128 else 32)
    g = torch.Generator().manual_seed(kpw)
    k8m, v8m = _codes((max_len, Hkv, D), g, cuda), _codes((max_len, Hkv, D), g, cuda)
    assert len(list(_attention_case(cuda, H, Hkv, kpw, 0, max_len, [pos], g, k8m, v8m))) == 1


# ------------------------------------------------------------------ 2. every code through the conversion
@pytest.mark.parametrize("kpw", [128, 256])
def test_every_code_through_the_conversion(cuda, kpw):
    H, Hkv, max_len = 32, 8, 2304
    j, h, d = torch.arange(max_len)[:, None, None], torch.arange(Hkv)[None, :, None], torch.arange(D)[None, None, :]
    code = ((131 * j + 7 * d + 29 * h) & 0xFF).to(torch.uint8)
    code[(code & 0x7F) == NAN8] = 0
    assert len(set(code[:258].flatten().tolist())) == 254        # all finite codes, already below the first position
    code = code.to(cuda)
    g = torch.Generator().manual_seed(kpw)
    for pos, q, k8, v8, got in _attention_case(cuda, H, Hkv, kpw, 0, max_len, [257, 1000, 2200], g, code, code, qstd=2.0 ** -8):
        # the premise, on the fp32 reference: no key hides behind a one-hot softmax
        kf = _deq(k8[:pos + 1]).float().repeat_interleave(H // Hkv, dim=1)               # [pos + 1, H, D]
        s = torch.einsum("hd,jhd->hj", q.view(H, D).float(), kf) * D ** -0.5
        w = torch.softmax(s, dim=1)
        print(f"pos {pos} kpw {kpw}: largest softmax weight {float(w.max()):.4f}")
        assert float(w.max()) < 0.25, pos


# ------------------------------------------------------------------ 3. q|k|v + RoPE + append, single row
def _rope_rows(max_len, cuda, theta=500000.0):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2).float() / D))
    fr = torch.arange(max_len).float()[:, None] * inv[None]
    return fr.cos().to(cuda).contiguous(), fr.sin().to(cuda).contiguous()


@functools.lru_cache(maxsize=None)
def _projection(H, Hkv, K, cuda):
    """q|k|v weight (made once per shape and shared) whose rows span 2^-18 .. 2^4 in scale — the RMSNorm in front fixes the scale of x itself, so
    the range comes from the weights: the projected key / value elements run from far below the format's flush threshold to beyond its saturation"""
    N = (H + 2 * Hkv) * D
    g = torch.Generator().manual_seed(H + Hkv + K)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.rand(N, 1, generator=g) * 22 - 18)
    nw = 1.0 + 0.1 * torch.randn(K, generator=g)
    return w.to(torch.bfloat16).to(cuda), nw.to(cuda)


def _sentinel(shape, cuda, salt):
    n = int(np.prod(shape))
    s = ((torch.arange(n) * 37 + salt) & 0xFF).to(torch.uint8)
    s[(s & 0x7F) == NAN8] = 1
    return s.view(shape).to(cuda)


@pytest.mark.parametrize("K", [4096, 2048])
@pytest.mark.parametrize("heads", [(32, 8), (8, 8), (16, 2)], ids=lambda h: f"{h[0]}x{h[1]}")
def test_qkv_rope_appends_the_quantised_row(cuda, heads, K):
    from videoglamm_amd import _lib, ops
    H, Hkv = heads
    max_len, eps = 512, 1e-5
    g = torch.Generator().manual_seed(H * Hkv + K)
    w, nw = _projection(H, Hkv, K, cuda)
    cos, sin = _rope_rows(max_len, cuda)
    big = small = False
    for pos in (0, 1, 77, max_len - 1):
        x = torch.randn(1, K, generator=g).to(torch.bfloat16).to(cuda)
        rope_cs = torch.cat([cos[pos], sin[pos]]).contiguous()
        p = torch.tensor([pos], dtype=torch.int32, device=cuda)
        kb, vb = torch.zeros(max_len, Hkv, D, dtype=torch.bfloat16, device=cuda), torch.zeros(max_len, Hkv, D, dtype=torch.bfloat16, device=cuda)
        q_want = ops.decode_qkv_rope(x, w, nw, eps, kb, vb, rope_cs, p, H, Hkv, D)
        k8, v8 = _sentinel((max_len, Hkv, D), cuda, 3), _sentinel((max_len, Hkv, D), cuda, 11)
        k8_0, v8_0 = k8.clone(), v8.clone()
        q = ops.decode_qkv_rope_kv8(x, w, nw, eps, k8, v8, rope_cs, p, H, Hkv, D)
        assert torch.equal(q, q_want), pos
        assert torch.equal(k8[pos], _ref(kb[pos])) and torch.equal(v8[pos], _ref(vb[pos])), pos
        k8[pos], v8[pos] = k8_0[pos], v8_0[pos]
        assert torch.equal(k8, k8_0) and torch.equal(v8, v8_0), pos                      # every other byte keeps its sentinel
        ka = kb[pos].float().abs()
        big, small = big or bool((ka > 448).any()), small or bool(((ka > 0) & (ka < 2.0 ** -10)).any())
    assert big and small                                         # saturation and flush both ran in the epilogue
    if K == 2048:
        with pytest.raises(_lib.VGKernelError, match="vg_decode_qkv_rope_kv8"):      # fp32 activations: unsupported, and refused before any launch
            ops._decode_qkv_rope("vg_decode_qkv_rope_kv8", x.float(), w.float(), nw, eps, k8, v8, rope_cs, p, H, Hkv, D, None)
        assert torch.equal(k8, k8_0) and torch.equal(v8, v8_0)


# ------------------------------------------------------------------ 4. the rows forms against the single-row forms
@pytest.mark.parametrize("kpw", [128, 256])
@pytest.mark.parametrize("Ppre", [255, 256, 257])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_rows_equal_single_row(cuda, B, Ppre, kpw):
    from videoglamm_amd import ops
    from videoglamm_amd.prompts import slot_layout
    H, Hkv, K, max_len, eps = 32, 8, 4096, 512, 1e-5
    g = torch.Generator().manual_seed(B * 1000 + Ppre + kpw)
    n_bound = Ppre + 80
    row0, _ = slot_layout(Ppre, kpw, n_bound)
    assert row0 == (0 if (Ppre, kpw) == (255, 256) else 128 if (Ppre, kpw) == (255, 128) else 256)
    slot_rows = n_bound - row0 + 3                               # slots longer than the bound: rows are scattered by a stride that is no block multiple
    # distinct positions (= distinct suffix lengths), the first slot row and the last row under the bound among them
    pos = [row0, n_bound - 1] + [int(p) for p in (row0 + 1 + torch.randperm(n_bound - row0 - 2, generator=g)[:B - 2])]
    assert len(set(pos)) == B
    w, nw = _projection(H, Hkv, K, cuda)
    cos, sin = _rope_rows(max_len, cuda)
    x = torch.randn(B, K, generator=g).to(torch.bfloat16).to(cuda)
    pk, pv = _codes((max_len, Hkv, D), g, cuda), _codes((max_len, Hkv, D), g, cuda)
    pk[row0:], pv[row0:] = NAN8, NAN8                            # the shared caches end at row0 for the rows kernel: never loaded behind it
    ks, vs = _codes((B, slot_rows, Hkv, D), g, cuda), _codes((B, slot_rows, Hkv, D), g, cuda)
    for b in range(B):
        ks[b, pos[b] - row0:], vs[b, pos[b] - row0:] = KMAX, VMIN
    ks0, vs0, pk0, pv0 = ks.clone(), vs.clone(), pk.clone(), pv.clone()
    pos_dev = torch.tensor(pos, dtype=torch.int32, device=cuda)
    rope_cs = torch.stack([torch.cat([cos[p], sin[p]]) for p in pos]).contiguous()
    ws = ops.decode_attention2_rows_workspace(H, Hkv, D, n_bound, kpw, B, cuda)
    q = ops.decode_qkv_rope_rows_kv8(x, w, nw, eps, ks, vs, row0, rope_cs, pos_dev, H, Hkv, D)
    o = ops.decode_attention2_rows_kv8(q, pk, pv, ks, vs, row0, H, Hkv, D, pos_dev, n_bound, D ** -0.5, ws, keys_per_wg=kpw)
    assert _counters(ws, B * Hkv) == 0 and bool(torch.isfinite(o.float()).all())
    assert torch.equal(pk, pk0) and torch.equal(pv, pv0)         # the shared prefix is read only
    ws1 = ops.decode_attention2_rows_workspace(H, Hkv, D, max_len, 128, 1, cuda)
    for r in range(B):
        kc, vc = pk0.clone(), pv0.clone()
        kc[row0:], vc[row0:] = KMAX, VMIN
        kc[row0:row0 + slot_rows], vc[row0:row0 + slot_rows] = ks0[r], vs0[r]
        p1 = torch.tensor([pos[r]], dtype=torch.int32, device=cuda)
        q1 = ops.decode_qkv_rope_kv8(x[r:r + 1].contiguous(), w, nw, eps, kc, vc, rope_cs[r].contiguous(), p1, H, Hkv, D)
        o1 = ops.decode_attention2_kv8(q1, kc, vc, H, Hkv, D, p1, D ** -0.5, ws1, keys_per_wg=kpw)
        assert torch.equal(q[r:r + 1], q1) and torch.equal(o[r:r + 1], o1), r
        # row r's append landed in slot r at its own position, and nothing else in the slot moved
        assert torch.equal(ks[r], kc[row0:row0 + slot_rows]) and torch.equal(vs[r], vc[row0:row0 + slot_rows]), r
        assert not torch.equal(ks[r], ks0[r]) and not torch.equal(vs[r], vs0[r]), r
    assert _counters(ws1, Hkv) == 0


# ------------------------------------------------------------------ 5. the decoder against a bf16-K/V rope-step decoder with e4m3-rounded cache rows
def _round_rows(dec, a, b):
    for i in range(len(dec.kc)):
        dec.kc[i][a:b] = _deq(_ref(dec.kc[i][a:b]))
        dec.vc[i][a:b] = _deq(_ref(dec.vc[i][a:b]))


@pytest.mark.parametrize("gemv", [None, "mfma", "mfma_q"])
def test_decoder_equals_rope_decoder_on_rounded_cache(cuda, monkeypatch, gemv):
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = llama._llm(cuda)
    c = cfg["llm"] if gemv is None else dict(cfg["llm"], decode_gemv=gemv)
    if gemv == "mfma_q":
        c = dict(c, decode_weights="fp8")
    S, steps = 70, 7
    ids = torch.randint(10, 8000, (S,), generator=torch.Generator().manual_seed(7)).to(cuda)
    x = ops.embed(ids, P.t("model.embed_tokens.weight"))
    # the twin's step rounds the row it appended before its attention reads it: what the mode's own step does by construction
    plain = ops.decode_qkv_rope

    def rounding(x_, wqkv, norm_w, eps, k_cache, v_cache, rope_cs, pos_dev, *a, **kw):
        q = plain(x_, wqkv, norm_w, eps, k_cache, v_cache, rope_cs, pos_dev, *a, **kw)
        p = int(pos_dev)
        k_cache[p] = _deq(_ref(k_cache[p]))
        v_cache[p] = _deq(_ref(v_cache[p]))
        return q

    monkeypatch.setattr(ops, "decode_qkv_rope", rounding)
    twin = LlamaDecoder(P, c, 1024, use_graph=False)
    dec = LlamaDecoder(P, dict(c, kv_cache="fp8_rope"), 1024, use_graph=False)
    rep = LlamaDecoder(P, dict(c, kv_cache="fp8_rope"), 1024, use_graph=True)
    assert dec.kv8 == "rope" and dec.rope_path and not dec.chain_roles and not twin.kv8 and twin.rope_path and twin.kc8 is None
    assert dec.mfma == (gemv == "mfma") and dec.mfma_q == (gemv == "mfma_q") and twin.mfma == dec.mfma and twin.mfma_q == dec.mfma_q
    assert dec.kc8[0].dtype == torch.uint8 and dec.kc8[0].shape == dec.kc[0].shape
    toks = {}
    for name, d in (("twin", twin), ("dec", dec), ("rep", rep)):
        d.reset()
        d.next_token(d.forward(x)[-1:])
        toks[name] = [int(d.tok_dev)]
    _round_rows(twin, 0, S)
    assert torch.equal(dec.hid_all[:S], twin.hid_all[:S])        # the prefill attends to unquantised K/V: today's launches
    for i in range(c["num_layers"]):
        assert torch.equal(dec.kc8[i][:S], _ref(dec.kc[i][:S])) and torch.equal(_deq(dec.vc8[i][:S]), twin.vc[i][:S])
    for s in range(steps):
        for name, d in (("twin", twin), ("dec", dec), ("rep", rep)):
            d.decode_step()
            toks[name].append(int(d.tok_dev))
        assert torch.equal(dec.hid_all[S + s], twin.hid_all[S + s]), s
        for i in range(c["num_layers"]):
            assert torch.equal(_deq(dec.kc8[i][S + s]), twin.kc[i][S + s]) and torch.equal(_deq(dec.vc8[i][S + s]), twin.vc[i][S + s]), (s, i)
            assert torch.equal(rep.kc8[i][S + s], dec.kc8[i][S + s]) and torch.equal(rep.vc8[i][S + s], dec.vc8[i][S + s]), (s, i)
    assert toks["dec"] == toks["twin"] and toks["rep"] == toks["dec"] and rep.graphs and not dec.graphs
    assert torch.equal(rep.hid_all[:S + steps], dec.hid_all[:S + steps])
    # a prefill behind decode steps: the staging takes the decoded rows from the e4m3 cache (the prefilled rows stay unquantised there)
    assert dec.staged == S
    h = dec.forward(x[:5])
    assert dec.staged == S + steps + 5 and bool(torch.isfinite(h.float()).all())
    for i in range(c["num_layers"]):
        assert torch.equal(dec.kc[i][S:S + steps], twin.kc[i][S:S + steps]) and torch.equal(dec.vc[i][S:S + steps], twin.vc[i][S:S + steps])
        assert torch.equal(dec.kc8[i][S + steps:S + steps + 5], _ref(dec.kc[i][S + steps:S + steps + 5]))


def test_decoder_refusals(cuda, monkeypatch):
    import test_prompts_batched_phi3_gpu as phi3
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = llama._llm(cuda)
    c = dict(cfg["llm"], kv_cache="fp8_rope")
    monkeypatch.setenv("VG_DECODE_ROPE", "0")
    with pytest.raises(ValueError, match="rope step") as e:
        LlamaDecoder(P, c, 1024)
    assert "kv_cache = 'fp8'" in str(e.value)
    monkeypatch.delenv("VG_DECODE_ROPE")
    Pp, cp, _ = phi3._llm(cuda)
    with pytest.raises(ValueError, match="rope step"):           # Phi-3-mini width: the rope step does not cover it
        LlamaDecoder(Pp, dict(cp["llm"], kv_cache="fp8_rope"), 1024)
    monkeypatch.setenv("VG_DECODE_CHAIN", "1")
    with pytest.raises(ValueError, match="VG_DECODE_CHAIN"):
        LlamaDecoder(P, c, 1024)
    monkeypatch.delenv("VG_DECODE_CHAIN")
    monkeypatch.setenv("VG_DECODE_FUSED", "0")
    with pytest.raises(ValueError, match="fused decode kernels"):
        LlamaDecoder(P, c, 1024)
    monkeypatch.delenv("VG_DECODE_FUSED")
    with pytest.raises(ValueError, match="forward_sharded"):
        LlamaDecoder(P, c, 1024).forward_sharded(torch.zeros(8, c["hidden"], dtype=torch.bfloat16, device=cuda), None)


# ------------------------------------------------------------------ 6. the entry points (Llama-3 width, 2 layers)
@functools.lru_cache(maxsize=1)
def _micro(cuda):
    """test_kv8_gpu._micro's model (tiny towers and SAM2) with a 2-layer Llama-3-8B-width LLM in the mode; five clips of other frames and prompts"""
    from videoglamm_amd import synth
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    cfg = dict(seg_token_idx=4095, projector_depth=2,
               iv2=dict(img_size=224, patch_size=14, embed_dim=128, depth=3, num_heads=4, mlp_hidden=256),
               clip=dict(img_size=336, patch_size=14, hidden=128, mlp=256, num_layers=3, num_heads=4),
               llm=dict(synth.LLAMA3_8B, num_layers=2, vocab=4096, kv_cache="fp8_rope"),
               sam2=dict(image_size=256, trunk=dict(embed_dim=16, num_heads=1, stages=[1, 2, 3, 1], global_att_blocks=[4, 5],
                                                    window_spec=[8, 4, 8, 4], window_pos_embed_bkg_spatial_size=[7, 7])))
    sd = synth.device_state_dict(synth.manifest(cfg), cuda, torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    clips = []
    for b in range(5):
        te, T, n = 4 * (1 + b % 2), 2, (3 * b + 4) % 10       # (the video encoder takes 4-frame chunks)
        images, context = torch.randn(te, 3, 224, 224, generator=g).to(cuda), torch.randn(te, 3, 336, 336, generator=g).to(cuda)
        sam = torch.randn(T, 3, 256, 256, generator=g).to(cuda)
        ids = torch.cat([torch.tensor([1, 5, 6]), torch.full((te,), -200), torch.randint(3, 4000, (n,), generator=g)])
        clips.append(([images], [context], [sam], ids[None], [(256, 256)], [(40, 48)]))
    m = VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.bfloat16, device=cuda)
    seg = cfg["seg_token_idx"]
    m.token_hook = lambda step, tok: seg if step in (1, 3) else None
    return m, clips


def _same_masks(x, y):
    assert sorted(x) == sorted(y) and all(sorted(x[t]) == sorted(y[t]) for t in x)
    assert all(np.array_equal(x[t][k], y[t][k]) for t in x for k in x[t])


SAMPLED = dict(do_sample=True, top_k=20, top_p=0.9, temperature=0.8)


def _slots_are_bytes(m, B):
    dec = m.P._decoder
    rows = next(iter(dec._rows.values()))
    assert dec.kv8 == "rope" and dec.rope_path and rows.kv8 and not rows.attn_rows and rows.B == (2 if B == 2 else 8)
    assert all(t.element_size() == 1 and t.dtype == torch.uint8 for t in rows.ks + rows.vs)
    return rows


@pytest.mark.parametrize("B,kw", [(2, {}), (5, {}), (5, SAMPLED)], ids=["B2-greedy", "B5-greedy", "B5-sampled"])
def test_inference_clips_equals_its_loop(cuda, monkeypatch, B, kw):
    m, clips = _micro(cuda)
    kw = dict(kw, max_new_tokens=6)
    monkeypatch.setenv("VG_CLIPS_BATCHED", "0")
    torch.manual_seed(77)
    ref = m.inference_clips(clips[:B], **kw)
    monkeypatch.setenv("VG_CLIPS_BATCHED", "1")
    m.P._decoder.__dict__.pop("_rows", None)
    torch.manual_seed(77)
    got = m.inference_clips(clips[:B], **kw)
    rows = _slots_are_bytes(m, B)
    assert rows.row0 == 0 and rows.steps == 5
    assert len(got) == len(ref) == B
    for (o, s), (ro, rs) in zip(got, ref):
        assert torch.equal(o, ro) and len(s) == len(rs) == 1 and len(s[0]) > 0
        _same_masks(s[0], rs[0])


@pytest.mark.parametrize("B", [2, 5])
def test_inference_prompts_equals_its_loop(cuda, monkeypatch, B):
    m, clips = _micro(cuda)
    images, context, sam, ids0, resize, orig = clips[0]
    g = torch.Generator().manual_seed(B)
    head = ids0[0][:7]                                           # 3 text ids + the four visual placeholders of clip 0
    ids = [torch.cat([head, torch.randint(3, 4000, ((3 * b + 4) % 10,), generator=g)]) for b in range(B)]
    kw = dict(max_new_tokens=6, shared=True)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = m.inference_prompts(images, context, sam, ids, resize, orig, **kw)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    m.P._decoder.__dict__.pop("_rows", None)
    got = m.inference_prompts(images, context, sam, ids, resize, orig, **kw)
    rows = _slots_are_bytes(m, B)
    assert rows.row0 == 768 and rows.steps == 5                  # P = 3 + 4 * 208 = 835: three shared 256-key blocks from kc8 / vc8
    assert len(got[0]) == len(ref[0]) == B
    for o, ro in zip(got[0], ref[0]):
        assert torch.equal(o, ro)
    for s, rs in zip(got[1], ref[1]):
        assert len(s) > 0
        _same_masks(s, rs)
