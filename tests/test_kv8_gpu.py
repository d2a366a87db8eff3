"""The fp8 K/V cache of the decode step (cfg["llm"]["kv_cache"] = "fp8") on the HIP kernels.  e4m3 -> bf16 is exact, so everything here
is torch.equal: the quantiser against the format's torch statement, vg_decode_attention_kv8 against vg_decode_attention on the dequantised caches
(whose own accuracy test_attention_accuracy_gpu.py pins), the rows kernel against the single-row one, the decoder against a bf16-K/V decoder whose
cache rows are rounded to e4m3 behind its back, and the batched entry points against their sequential loops."""
import functools

import numpy as np
import pytest
import torch

import test_prompts_batched_gpu as llama
import test_prompts_batched_phi3_gpu as phi3

torch.set_grad_enabled(False)

pytestmark = pytest.mark.gpu

NAN8 = 0x7F


def _ref(x):
    """the format, as the issue states it"""
    return x.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _codes(shape, g, cuda, std=1.0):
    """random non-NaN e4m3 codes: N(0, std) rounded to the format"""
    return _ref((torch.randn(*shape, generator=g) * std).to(torch.bfloat16)).to(cuda)


# ------------------------------------------------------------------ 1. the quantiser
def test_quantiser_equals_the_torch_statement(cuda):
    from videoglamm_amd import ops
    finite = torch.tensor([c for c in range(256) if c & 0x7F != NAN8], dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    pos = finite[finite >= 0].sort().values
    mid = (pos[:-1] + pos[1:]) / 2                               # the ties: four mantissa bits, exact in bf16
    edge = torch.tensor([0.0, -0.0, 448.0, -448.0, 449.0, -449.0, 1e4, -1e4, 2.0 ** -9, 2.0 ** -10, 2.0 ** -11, float("nan")])
    rnd = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * torch.logspace(-3, 3, 4096)
    x32 = torch.cat([finite, mid, -mid, edge, -edge[8:11], rnd])
    x = x32.to(torch.bfloat16)
    assert torch.equal(x[:finite.numel() + 2 * mid.numel()].float(), x32[:finite.numel() + 2 * mid.numel()])      # held exactly
    x = x.to(cuda)
    want = _ref(x)
    assert torch.equal(want, ops.kv_quantize_reference(x))
    for n in (x.numel(), x.numel() - 1, x.numel() - 2, x.numel() - 3, 5, 4, 3, 1):      # whole dwords and every tail length
        dst = torch.full((x.numel() + 16,), 0xA5, dtype=torch.uint8, device=cuda)
        ops.kv_quantize_(x[:n], dst[:n])
        assert torch.equal(dst[:n], want[:n]), n
        assert bool((dst[n:] == 0xA5).all()), n                  # the sentinels behind n
    assert torch.equal(ops.kv_dequantize(want[:finite.numel()]).float().cpu(), finite)


# ------------------------------------------------------------------ 2. the attention against the bf16 kernel on the dequantised caches
SHAPES = [(32, 32, 96, 256, 0), (32, 32, 96, 256, 100), (32, 8, 128, 320, 0), (8, 2, 64, 192, 0), (4, 4, 96, 1024, 65)]
POSITIONS = [0, 1, 62, 63, 64, 65, 127, 128, 129, -1]


@functools.lru_cache(maxsize=1)
def _workspace(cuda):
    from videoglamm_amd import ops
    n = max(ops.decode_attention_workspace(H, Hkv, D, L, "cpu").numel() for H, Hkv, D, L, _ in SHAPES)
    return torch.zeros(n, dtype=torch.float32, device=cuda)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_equals_bf16_kernel_on_dequantised_cache(cuda, shape):
    from videoglamm_amd import ops
    H, Hkv, D, max_len, window = shape
    assert ops.decode_attention_kv8_supported(H, Hkv, D, torch.bfloat16) and not ops.decode_attention_kv8_supported(H, Hkv, D, torch.float32)
    g = torch.Generator().manual_seed(H * 1000 + D + window)
    k8m, v8m = _codes((max_len, Hkv, D), g, cuda), _codes((max_len, Hkv, D), g, cuda, 2.0)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.arange(max_len).float()[:, None] * inv[None]
    cos, sin = fr.cos().to(cuda).contiguous(), fr.sin().to(cuda).contiguous()
    # one workspace for every case, both kernels: the shape's floats of it, zero-filled once per shape (its counters sit at the shape's own offset)
    need = ops.decode_attention_workspace(H, Hkv, D, max_len, "cpu").numel()
    ws = _workspace(cuda)[:need]
    ws.zero_()
    for pos in POSITIONS:
        pos = pos % max_len
        for kpw in (0, 128):
            qkv = (torch.randn(1, (H + 2 * Hkv) * D, generator=g) * 1.5).to(torch.bfloat16).to(cuda)
            k8, v8 = k8m.clone(), v8m.clone()
            k8[pos:], v8[pos:] = NAN8, NAN8                      # row pos and everything behind it: poison until the append
            k8_0, v8_0 = k8.clone(), v8.clone()
            kb, vb = ops.kv_dequantize(k8), ops.kv_dequantize(v8)
            assert pos == max_len - 1 or bool(kb[pos + 1].isnan().all())
            p = torch.tensor([pos], dtype=torch.int32, device=cuda)
            got = ops.decode_attention_kv8(qkv, k8, v8, cos, sin, H, Hkv, D, p, D ** -0.5, ws, window=window, keys_per_wg=kpw)
            assert int(ws[need - Hkv:].view(torch.int32).abs().sum()) == 0, (pos, kpw)           # the arrival counters reset themselves
            want = ops.decode_attention(qkv, kb, vb, cos, sin, H, Hkv, D, p, D ** -0.5, ws, window=window, keys_per_wg=kpw)
            assert int(ws[need - Hkv:].view(torch.int32).abs().sum()) == 0, (pos, kpw)
            assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, want), (pos, kpw)
            # the appended row is the quantised form of the row the bf16 kernel appended; no other byte moved
            assert torch.equal(k8[pos], _ref(kb[pos])) and torch.equal(v8[pos], _ref(vb[pos])), (pos, kpw)
            assert not bool((k8[pos] == NAN8).any())
            k8[pos], v8[pos] = NAN8, NAN8
            assert torch.equal(k8, k8_0) and torch.equal(v8, v8_0), (pos, kpw)


# ------------------------------------------------------------------ 3. the B-row kernel against the single-row one
@pytest.mark.parametrize("kpw_min", [0, 8192])
@pytest.mark.parametrize("window", [0, 63, 200])
@pytest.mark.parametrize("Ppre", [300, 512, 520])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_attention_rows_equal_single_row(cuda, B, Ppre, window, kpw_min):
    from videoglamm_amd import ops
    from videoglamm_amd.prompts import slot_layout
    from videoglamm_amd.vlm import RowsDecode
    H = Hkv = 32
    D, max_len = 96, 1024
    assert ops.decode_attention_rows_kv8_supported(H, Hkv, D, torch.bfloat16) and not ops.decode_attention_rows_kv8_supported(32, 8, 128, torch.bfloat16)
    g = torch.Generator().manual_seed(B * 1000 + Ppre + window)
    n_bound = Ppre + 80
    row0, _ = slot_layout(Ppre, RowsDecode.ATTN_KW, n_bound)
    pos = [row0, n_bound - 1] + [int(p) for p in (row0 + 1 + torch.randperm(n_bound - row0 - 2, generator=g)[:B - 2])]
    assert len(set(pos)) == B
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.arange(max_len).float()[:, None] * inv[None]
    cos, sin = fr.cos().to(cuda).contiguous(), fr.sin().to(cuda).contiguous()
    pk, pv = _codes((max_len, Hkv, D), g, cuda), _codes((max_len, Hkv, D), g, cuda, 2.0)
    pk[row0:], pv[row0:] = NAN8, NAN8                            # the shared caches end at row0 for the kernel
    ks, vs = _codes((B, n_bound - row0, Hkv, D), g, cuda), _codes((B, n_bound - row0, Hkv, D), g, cuda, 2.0)
    for b in range(B):
        ks[b, pos[b] - row0:], vs[b, pos[b] - row0:] = NAN8, NAN8
    ks0, vs0, pk0, pv0 = ks.clone(), vs.clone(), pk.clone(), pv.clone()
    qkv = (torch.randn(B, (H + 2 * Hkv) * D, generator=g) * 1.5).to(torch.bfloat16).to(cuda)
    pos_dev = torch.tensor(pos, dtype=torch.int32, device=cuda)
    ws = ops.decode_attention_rows_workspace(H, Hkv, D, n_bound, B, cuda)
    o = ops.decode_attention_rows_kv8(qkv, pk, pv, ks, vs, row0, cos, sin, H, Hkv, D, pos_dev, n_bound, D ** -0.5, ws, window=window, kpw_min=kpw_min)
    assert int(ws[ws.numel() - B * Hkv:].view(torch.int32).abs().sum()) == 0
    assert bool(torch.isfinite(o.float()).all())
    assert torch.equal(pk, pk0) and torch.equal(pv, pv0)         # the shared prefix is read only
    ws1 = ops.decode_attention_workspace(H, Hkv, D, max_len, cuda)
    for r in range(B):
        kc, vc = pk0.clone(), pv0.clone()
        kc[row0:n_bound], vc[row0:n_bound] = ks0[r], vs0[r]
        p1 = torch.tensor([pos[r]], dtype=torch.int32, device=cuda)
        o1 = ops.decode_attention_kv8(qkv[r:r + 1].contiguous(), kc, vc, cos, sin, H, Hkv, D, p1, D ** -0.5, ws1, window=window,
                                      keys_per_wg=128 if pos[r] >= kpw_min else 0)
        assert torch.equal(o[r:r + 1], o1), r
        # row r's append landed in slot r at its own position, and nothing else in the slot moved
        assert torch.equal(ks[r], kc[row0:n_bound]) and torch.equal(vs[r], vc[row0:n_bound]), r
        assert not bool((ks[r, pos[r] - row0] == NAN8).any()) and not torch.equal(ks[r], ks0[r]), r


# ------------------------------------------------------------------ 4. the decoder against a bf16-K/V decoder with e4m3-rounded cache rows
def _round_rows(dec, a, b):
    from videoglamm_amd import ops
    for i in range(len(dec.kc)):
        dec.kc[i][a:b] = ops.kv_dequantize(_ref(dec.kc[i][a:b]))
        dec.vc[i][a:b] = ops.kv_dequantize(_ref(dec.vc[i][a:b]))


@pytest.mark.parametrize("width", ["phi3", "llama"])
def test_decoder_equals_bf16_decoder_on_rounded_cache(cuda, monkeypatch, width):
    from videoglamm_amd import ops
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = (phi3 if width == "phi3" else llama)._llm(cuda)
    c = cfg["llm"]
    S, steps = 70, 7
    ids = torch.randint(10, 8000, (S,), generator=torch.Generator().manual_seed(7)).to(cuda)
    x = ops.embed(ids, P.t("model.embed_tokens.weight"))
    monkeypatch.setenv("VG_DECODE_ROPE", "0")                    # the twin on the decode_attention step (Llama-3 width would take the rope step)
    twin = LlamaDecoder(P, c, 1024, use_graph=False)
    monkeypatch.delenv("VG_DECODE_ROPE")
    dec = LlamaDecoder(P, dict(c, kv_cache="fp8"), 1024, use_graph=False)
    rep = LlamaDecoder(P, dict(c, kv_cache="fp8"), 1024, use_graph=True)
    assert dec.kv8 and not dec.rope_path and not dec.chain_roles and not twin.kv8 and not twin.rope_path and twin.kc8 is None
    assert dec.kc8[0].dtype == torch.uint8 and dec.kc8[0].shape == dec.kc[0].shape
    toks = {}
    for name, d in (("twin", twin), ("dec", dec), ("rep", rep)):
        d.reset()
        d.next_token(d.forward(x)[-1:])
        toks[name] = [int(d.tok_dev)]
    _round_rows(twin, 0, S)
    assert torch.equal(dec.hid_all[:S], twin.hid_all[:S])        # the prefill attends to unquantised K/V: today's launches
    for i in range(c["num_layers"]):
        assert torch.equal(dec.kc8[i][:S], _ref(dec.kc[i][:S])) and torch.equal(ops.kv_dequantize(dec.vc8[i][:S]), twin.vc[i][:S])
    for s in range(steps):
        for name, d in (("twin", twin), ("dec", dec), ("rep", rep)):
            d.decode_step()
            toks[name].append(int(d.tok_dev))
        _round_rows(twin, S + s, S + s + 1)
        assert torch.equal(dec.hid_all[S + s], twin.hid_all[S + s]), s
        for i in range(c["num_layers"]):
            assert torch.equal(ops.kv_dequantize(dec.kc8[i][S + s]), twin.kc[i][S + s]), (s, i)
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
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, _ = llama._llm(cuda)
    c = dict(cfg["llm"], kv_cache="fp8")
    for gemv in ("mfma", "mfma_q"):
        with pytest.raises(ValueError, match="decode_gemv"):
            LlamaDecoder(P, dict(c, decode_gemv=gemv, decode_weights="fp8" if gemv == "mfma_q" else None), 1024)
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
    Pp, cp, _ = phi3._llm(cuda)
    assert LlamaDecoder(Pp, dict(cp["llm"], kv_cache="fp8", decode_gemv="mfma"), 1024).mfma       # Phi-3-mini width keeps its rows step


# ------------------------------------------------------------------ 5. the entry points (Phi-3-mini width, 2 layers)
@functools.lru_cache(maxsize=1)
def _micro(cuda):
    """the micro model (tiny towers and SAM2) with a 2-layer Phi-3-mini-width LLM in the mode; five clips of other frames and prompts"""
    from videoglamm_amd import synth
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    cfg = dict(seg_token_idx=4095, projector_depth=2,
               iv2=dict(img_size=224, patch_size=14, embed_dim=128, depth=3, num_heads=4, mlp_hidden=256),
               clip=dict(img_size=336, patch_size=14, hidden=128, mlp=256, num_layers=3, num_heads=4),
               llm=dict(synth.PHI3_MINI, num_layers=2, vocab=4096, sliding_window=199, kv_cache="fp8"),
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
    rows = next(iter(m.P._decoder._rows.values()))
    assert m.P._decoder.kv8 and rows.kv8 and rows.attn_rows and rows.B == (2 if B == 2 else 8)
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


@pytest.mark.parametrize("B,kw", [(2, {}), (5, {}), (5, SAMPLED)], ids=["B2-greedy", "B5-greedy", "B5-sampled"])
def test_inference_prompts_equals_its_loop(cuda, monkeypatch, B, kw):
    m, clips = _micro(cuda)
    images, context, sam, ids0, resize, orig = clips[0]
    g = torch.Generator().manual_seed(B)
    head = ids0[0][:7]                                           # 3 text ids + the four visual placeholders of clip 0
    ids = [torch.cat([head, torch.randint(3, 4000, ((3 * b + 4) % 10,), generator=g)]) for b in range(B)]
    kw = dict(kw, max_new_tokens=6, shared=True)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    torch.manual_seed(78)
    ref = m.inference_prompts(images, context, sam, ids, resize, orig, **kw)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    m.P._decoder.__dict__.pop("_rows", None)
    torch.manual_seed(78)
    got = m.inference_prompts(images, context, sam, ids, resize, orig, **kw)
    rows = _slots_are_bytes(m, B)
    assert rows.row0 == 768 and rows.steps == 5                  # P = 3 + 4 * 208 = 835: six shared 128-key blocks from kc8 / vc8
    assert len(got[0]) == len(ref[0]) == B
    for o, ro in zip(got[0], ref[0]):
        assert torch.equal(o, ro)
    for s, rs in zip(got[1], ref[1]):
        assert len(s) > 0
        _same_masks(s, rs)
