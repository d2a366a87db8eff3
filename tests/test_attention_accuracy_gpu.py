"""Every bf16 attention kernel against float64, with a bound taken from the arithmetic instead of from the signal (-m gpu).

The older attention tests compare flat-softmax outputs (|o| ~ 0.02 .. 0.07) with atol = 2e-2: a dropped, doubled or leaked key passes them.
Here (tests/_attn_ref.py):
  * reference: the suite's statement in float64 on the same bf16 operands;
  * metric: per (batch, head, query row) ||got - ref||_2 / ||ref||_2 over the head dim;
  * bound: K_BOUND x the maximum row error of the honest bf16 flash model (fp32 scores and softmax, exp(s - m) rounded to bf16 before P.V, fp32
    accumulation and row sum, bf16 output) on the SAME inputs, computed on the CPU in the test;
  * inputs: random q/k/v plus probe rows (at most 25 % of the rows) in which one chosen key holds >= 50 % of the softmax mass — the first and
    last keys, both sides of every 64- / 128- / 256-key and split-KV boundary, the diagonal key of the rows beside every query-tile edge, the
    oldest key inside a sliding window — and negative probes on the first masked keys (diag + 1, diag - window), asserted on the CPU.
tests/test_attention_accuracy_selfcheck.py proves on the CPU that each of eleven wrong kernels fails this bound where the honest model passes.

Shapes are those of the older tests (ATT, WIN, test_attention_dma_gpu's lists, test_attention_dv, the window and the decode tests).  Routes: the
library has no query for the route vg_attention takes, so _route() restates the thresholds (ops.attention: KV split when fewer than 384 query
blocks and Skv >= 512; vg_attention_dma.hip attn_dma_eligible: bf16, 32 < D <= 128, no split, no fold, no window, Sq >= 512 with at most 1/8 of
the padded 256-row tiles idle) and the cases that are meant for a route assert it there.  By that rule most shapes of
test_attention_dma_vs_fp32_statement take the split-KV route of attn_kernel through ops.attention (few heads: fewer than 384 blocks), so the
"dma" cases below carry enough heads or batch entries to reach the LDS-DMA kernel unsplit.

Measured (also DESIGN.md section 2) — max row_err(kernel) / max row_err(model) per case, measured on the MI355X (model's own maximum: 2.5e-3 .. 5.0e-3 in every case):
  ops.attention, generic route (ATT, WIN, fused q|k|v views; 10 cases)            1.00 .. 1.49  (largest: 32 x 3361 x 3361, d = 96, window 2048)
  ops.attention, split-KV + merge (20 cases, incl. causal offset, GQA, window)      1.00 .. 1.62  (largest: 700 x 700, d = 96, window 100)
  ops.attention, LDS-DMA kernel (7 cases, incl. 32 x 3361 x 3361 causal, d = 128)   1.10 .. 1.44
  ops.attention_dv (10 cases; split and unsplit, Sq < 256 and >= 256)               1.00 .. 1.75  (largest: 4096 x 28 736, 16 splits)
  ops.attention_windows / ops.window_attention (15 cases)                           1.00 .. 1.13
  ops.attention_decode (11 cases)                                                   0.88 .. 1.04
  ops.decode_attention2 (16 cases), ops.decode_attention2_rows (4 cases)            0.89 .. 1.00
  ops.decode_attention (22 cases: 64 and 128 keys per workgroup)                    1.23 .. 2.36  (*)
  ops.decode_attention_rows (18 cases)                                              1.76 .. 3.21  (*)
K_BOUND = 4: twice the largest ratio of the kernels that are handed their operands (1.75 -> 3.5), rounded up to one digit.
(*) a finding, not folded into K_BOUND: these two kernels rotate q and the new key themselves, in vg_rope_kv_append's arithmetic (cos / sin rounded
to bf16, every product rounded to bf16), while the reference here rotates in fp32 on the fp32 tables and rounds once; a probe row's logit is ~ 9,
so the rotation's rounding shows.  The figures are identical for 64 and 128 keys per workgroup, and the same attention fed pre-rotated operands
(attention_decode, decode_attention2) sits at <= 1.04: the excess is the RoPE's, not the softmax's, split's or merge's.  Both kernels pass at
K_BOUND = 4; twice their largest ratio would be 6.4.
"""
import pytest
import torch

import _attn_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

def _route(B, Hq, Hkv, Sq, Skv, D, causal, window):
    """(route, split edges) ops.attention takes in bf16 — a restatement of its thresholds, see the module docstring"""
    from videoglamm_amd import ops
    blocks = -(-Sq // 128) * Hq * B
    nsplit = 1
    if Skv >= 512 and blocks < 384:
        nsplit = max(1, min(64, (ops._SPLIT_WG_D256 if D > 128 else 512) // blocks, Skv // 128))
    if nsplit > 1:
        L = (-(-Skv // nsplit) + 63) // 64 * 64
        return "split", list(range(L, Skv, L))
    fold = Hq > Hkv and (Hq // Hkv) * Sq <= 128
    padded = -(-Sq // 256) * 256
    dma = 32 < D <= 128 and not fold and not window and Sq >= 512 and (Sq >= 1024 or (padded - Sq) * 8 <= padded)
    return ("dma" if dma else "generic"), []


def _check(name, cases, kernel):
    ek, em = R.evaluate(cases, kernel)
    ratio = float(ek.max()) / max(float(em.max()), 1e-30)
    print(f"ACC {name:60s} kernel {float(ek.max()):9.3e} model {float(em.max()):9.3e} ratio {ratio:6.2f} rounds {len(cases)}")
    assert R.passes(ek, em), (name, float(ek.max()), float(em.max()), ratio)


# ------------------------------------------------------------------ ops.attention
PREFILL = [  # B, Hq, Hkv, Sq, Skv, D, causal, window, route meant (None: whatever the rule gives), checked KV groups (None: all)
    # ATT (test_kernels_gpu.py)
    (1, 2, 2, 64, 64, 72, False, 0, "generic", None), (2, 4, 4, 16, 64, 72, False, 0, "generic", None),
    (1, 16, 16, 1025, 1025, 88, False, 0, None, None), (2, 16, 16, 577, 577, 64, False, 0, None, None),
    (1, 8, 8, 7, 4096, 16, False, 0, "split", None), (2, 8, 8, 4096, 9, 16, False, 0, "generic", None), (1, 8, 8, 7, 7, 32, False, 0, "generic", None),
    (1, 1, 1, 1024, 1024, 256, False, 0, "split", None), (1, 1, 1, 1024, 2100, 256, False, 0, "split", None),
    (1, 8, 2, 333, 333, 128, True, 0, "generic", None), (1, 8, 2, 1, 700, 128, True, 0, "split", None), (1, 4, 4, 100, 100, 96, True, 0, "generic", None),
    (1, 4, 4, 33, 160, 64, True, 0, "generic", None), (1, 32, 8, 213, 1697, 128, True, 0, "split", None), (1, 32, 8, 849, 1697, 128, True, 0, "split", None),
    # test_attention_dma_gpu.py's list as it stands (split-KV by the rule, except the last) ...
    (1, 8, 2, 1300, 1300, 128, True, 0, "split", None), (1, 4, 4, 600, 777, 128, True, 0, "split", None), (1, 4, 4, 513, 513, 128, False, 0, "split", None),
    (2, 4, 4, 1024, 1024, 72, False, 0, "split", None), (1, 2, 2, 4096, 4096, 72, False, 0, "split", None), (3, 4, 4, 1025, 1025, 64, False, 0, "split", None),
    (2, 4, 4, 1025, 1025, 88, False, 0, "split", None), (1, 2, 2, 700, 70, 96, False, 0, "dma", None),
    # ... and with enough heads / batch entries for the LDS-DMA kernel (>= 384 query blocks, no split; 600 rows leave more than 1/8 of three
    # 256-row tiles idle and never go there), and the full-size causal prefill
    (5, 8, 2, 1300, 1300, 128, True, 0, "dma", None), (1, 12, 12, 4096, 4096, 72, False, 0, "dma", [0, 5, 11]),
    (6, 8, 8, 1025, 1025, 64, False, 0, "dma", None), (6, 8, 8, 1025, 1025, 88, False, 0, "dma", None),
    (1, 32, 8, 3361, 3361, 128, True, 0, "dma", [0, 3, 7]),
    # WIN (test_kernels_gpu.py): causal + sliding window
    (1, 4, 4, 700, 700, 96, True, 100, None, None), (1, 4, 4, 700, 700, 96, True, 257, None, None), (1, 8, 2, 333, 333, 128, True, 64, None, None),
    (1, 4, 4, 213, 1697, 96, True, 300, "split", None), (1, 4, 4, 1, 700, 96, True, 130, "split", None),
    (1, 32, 32, 3361, 3361, 96, True, 2048, "generic", [0, 13, 31]),      # the released model at NUM_FRAMES = 16, checked on three heads
]


@pytest.mark.parametrize("cfg", PREFILL, ids=lambda c: "-".join(str(x) for x in c[:8]))
def test_attention(cuda, cfg):
    from videoglamm_amd import ops
    B, Hq, Hkv, Sq, Skv, D, causal, window, meant, groups = cfg
    route, edges = _route(B, Hq, Hkv, Sq, Skv, D, causal, window)
    assert meant is None or route == meant, (route, meant)
    cases = R.all_rounds(B, Hq, Hkv, Sq, Skv, D, causal=causal, window=window, seed=1, split_edges=edges, groups=groups)

    def kernel(c):
        o = ops.attention(c["q"].to(cuda), c["k"].to(cuda), c["v"].to(cuda), c["scale"], causal, window=window)
        return R.checked(c, o.cpu())
    _check(f"attention {route} {cfg[:8]}", cases, kernel)


@pytest.mark.parametrize("B,S,H,D", [(2, 1025, 4, 88), (6, 1025, 8, 88), (2, 200, 4, 72)])
def test_attention_fused_qkv_views(cuda, B, S, H, D):
    """q, k, v as strided views of ONE fused projection [B, S, 3, H, D] (test_attention_dma_strided_fused_qkv, test_attention_fused_qkv_strides_and_spike)"""
    from videoglamm_amd import ops
    route, edges = _route(B, H, H, S, S, D, False, 0)
    assert route == {2: "split", 6: "dma"}[B] if S > 512 else route == "generic"
    cases = R.all_rounds(B, H, H, S, S, D, seed=2, split_edges=edges)

    def kernel(c):
        g = torch.stack([c["q"], c["k"], c["v"]], dim=2).to(cuda)
        assert not g[:, :, 1].is_contiguous()
        return R.checked(c, ops.attention(g[:, :, 0], g[:, :, 1], g[:, :, 2], c["scale"]).cpu())
    _check(f"attention fused-qkv {route} {(B, S, H, D)}", cases, kernel)


# ------------------------------------------------------------------ ops.attention_dv
@pytest.mark.parametrize("B,Sq,Skv,rows,batches", [
    (1, 1024, 2100, None, None), (2, 320, 700, None, None), (1, 4096, 4096 + 4, None, None),            # test_attention_dv
    (8, 4096, 7 * 4096 + 64, (100, 612), [0, 7]),                                                       # the full-size shape on the existing slice
    (1, 4096, 7 * 4096 + 64, (100, 612), None), (2, 300, 1000, None, None), (1, 256, 130, None, None), (3, 511, 64, None, None),   # test_attention_dma_gpu
    (1, 192, 1024 + 63, None, None), (1, 192, 64 + 28, None, None),                                     # test_attention_dv_every_tail: Sq < 256, split / one split
])
def test_attention_dv(cuda, B, Sq, Skv, rows, batches):
    """vg_attention_dv in bf16 (D = 256, DV = 64): Sq >= 256 takes attn_dma_d256v64_kernel, below attn_kernel's key-split form (ops.attention_dv's
    rule, restated: 256- / 128-row blocks, KV split when fewer than 384 blocks and Skv >= 512, aiming at 256 workgroups)"""
    from videoglamm_amd import ops
    D, DV = 256, 64
    blocks = -(-Sq // (256 if Sq >= 256 else 128)) * B
    nsplit = max(1, min(64, ops._SPLIT_WG_D256 // blocks, Skv // 128)) if Skv >= 512 and blocks < 384 else 1
    L = (-(-Skv // nsplit) + 63) // 64 * 64
    assert (nsplit > 1) == (Skv >= 512)
    cases = R.all_rounds(B, 1, 1, Sq, Skv, D, DV=DV, seed=3, split_edges=range(L, Skv, L) if nsplit > 1 else (), rows=rows, batches=batches)

    def kernel(c):
        o = ops.attention_dv(c["q"].to(cuda), c["k"].to(cuda), c["v"].to(cuda), c["scale"])
        assert o.shape == (B, Sq, 1, DV)
        return R.checked(c, o.cpu())
    _check(f"attention_dv nsplit={nsplit} {(B, Sq, Skv)}", cases, kernel)


# ------------------------------------------------------------------ Hiera's window kernels
@pytest.mark.parametrize("Bw,wtok,H,D", [(64, 16, 4, 72), (8, 64, 2, 72), (6, 16, 2, 32), (16, 49, 4, 72), (24, 32, 1, 64),
                                         (5, 256, 8, 72), (3, 256, 2, 64), (2, 256, 3, 80), (33, 256, 8, 72)])
def test_attention_windows(cuda, Bw, wtok, H, D):
    """test_attention_windows' list: vg_window_attention where it takes the shape (D = 72 at 16 / 64 tokens, 256-token windows), the packed
    block-diagonal vg_attention (wtok < 128, a window count that packs), the plain fallback otherwise"""
    from videoglamm_amd import ops
    cases = R.all_rounds(Bw, H, H, wtok, wtok, D, seed=4)

    def kernel(c):
        g = torch.stack([c["q"], c["k"], c["v"]], dim=2).to(cuda)
        dedicated = ops.window_attention(g[:, :, 0], g[:, :, 1], g[:, :, 2], c["scale"]) is not None
        assert dedicated == ((wtok in (16, 64) and D == 72) or wtok == 256)
        return R.checked(c, ops.attention_windows(g[:, :, 0], g[:, :, 1], g[:, :, 2], c["scale"]).cpu())
    _check(f"attention_windows {(Bw, wtok, H, D)}", cases, kernel)


@pytest.mark.parametrize("Bw,wq,wk,H", [(37, 4, 16, 8), (64, 16, 64, 4), (5, 16, 16, 3), (9, 64, 64, 2), (1024, 16, 16, 4), (300, 64, 64, 16)])
def test_window_attention_small(cuda, Bw, wq, wk, H):
    """test_window_attention_small's list: one wave per (window, head); q its own tensor where pooled, k / v strided views of a fused projection"""
    from videoglamm_amd import ops
    cases = R.all_rounds(Bw, H, H, wq, wk, 72, seed=5)

    def kernel(c):
        g = torch.stack([c["k"], c["k"], c["v"]], dim=2).to(cuda)
        o = ops.window_attention(c["q"].to(cuda), g[:, :, 1], g[:, :, 2], c["scale"])
        assert o is not None
        return R.checked(c, o.cpu())
    _check(f"window_attention {(Bw, wq, wk, H)}", cases, kernel)


# ------------------------------------------------------------------ decode steps
def _tables(max_len, D, theta=10000.0):
    ang = torch.arange(max_len)[:, None].float() * (1.0 / (theta ** (torch.arange(0, D, 2).float() / D)))[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def _fused(c, cos, sin):
    """a one-row case for the kernels that rotate q and the new key themselves: the case's q / k become the RAW projections — the caches hold every
    key rotated at the step's position (a rotation keeps the dot products, so the probes stay probes; check_probes runs on the rotated values),
    the new key and value travel in the q|k|v row and the cache rows at pos start as zeros"""
    pos, (H, D), Hkv = c["pos_i"], c["q"].shape[2:], c["k"].shape[2]
    kc = R.rope_rows(c["k_cache"], cos, sin, pos)
    qkv = torch.cat([c["q"][0, 0].reshape(-1), c["k_cache"][pos].reshape(-1), c["v_cache"][pos].reshape(-1)])[None].contiguous()
    f = dict(c, q=R.rope_rows(c["q"][0, 0], cos, sin, pos)[None, None], k=kc[None, : pos + 1], qkv=qkv, k_cache=kc.clone(), v_cache=c["v_cache"].clone())
    f["k_cache"][pos], f["v_cache"][pos] = 0, 0
    return f


DECODE = [(8, 2, 64, 640, 0), (32, 8, 128, 2048, 0), (4, 2, 16, 128, 0), (4, 4, 96, 256, 0), (8, 1, 32, 192, 0), (32, 32, 96, 2048, 0),      # test_decode_attention
          (4, 4, 96, 1024, 100), (4, 4, 96, 1024, 64), (4, 4, 96, 1024, 65), (32, 8, 128, 2048, 700), (32, 32, 96, 4096, 2048)]             # ..._sliding_window


@pytest.mark.parametrize("H,Hkv,D,max_len,window", DECODE)
def test_attention_decode(cuda, H, Hkv, D, max_len, window):
    """ops.attention_decode (vg_attention_splitkv with the device-side length): one 64-key tile per workgroup, the valid length read on the device"""
    from videoglamm_amd import ops
    cases = [c for pos in R.decode_positions(max_len, window) for c in R.decode_rounds(H, Hkv, D, max_len, pos, window, seed=6)]

    def kernel(c):
        pos_dev = torch.tensor([c["pos_i"]], dtype=torch.int32, device=cuda)
        return ops.attention_decode(c["q"].to(cuda), c["k_cache"].to(cuda), c["v_cache"].to(cuda), pos_dev, c["scale"], window=window).cpu()
    _check(f"attention_decode {(H, Hkv, D, max_len, window)}", cases, kernel)


@pytest.mark.parametrize("kpw", [0, 128])
@pytest.mark.parametrize("H,Hkv,D,max_len,window", DECODE)
def test_decode_attention(cuda, H, Hkv, D, max_len, window, kpw):
    """ops.decode_attention (RoPE + append + split attention + merge in one launch) on ONE replayed workspace; keys_per_wg = 128 is honoured for
    (G = 4, d = 128) and (MHA, d = 96) (vg_decode.hip: launch_decode_attn), the 64-key kernel runs elsewhere; the appended rows are checked too"""
    from videoglamm_amd import ops
    cos, sin = _tables(max_len, D)
    g_cos, g_sin = cos.to(cuda), sin.to(cuda)
    ws = ops.decode_attention_workspace(H, Hkv, D, max_len, cuda)
    cases = [_fused(c, cos, sin) for pos in R.decode_positions(max_len, window) for c in R.decode_rounds(H, Hkv, D, max_len, pos, window, seed=7)]

    def kernel(c):
        pos = c["pos_i"]
        kc, vc = c["k_cache"].to(cuda), c["v_cache"].to(cuda)
        o = ops.decode_attention(c["qkv"].to(cuda), kc, vc, g_cos, g_sin, H, Hkv, D, torch.tensor([pos], dtype=torch.int32, device=cuda), c["scale"], ws,
                                 window=window, keys_per_wg=kpw)
        assert torch.equal(vc[pos].cpu(), c["v"][0, pos]) and (kc[pos].cpu().float() - c["k"][0, pos].float()).abs().max() <= 2 ** -7 * c["k"][0, pos].float().abs().max()
        return o.view(1, 1, H, D).cpu()
    _check(f"decode_attention kpw={kpw} {(H, Hkv, D, max_len, window)}", cases, kernel)
    assert int(ws[-Hkv:].view(torch.int32).abs().sum()) == 0      # the arrival counters reset themselves


@pytest.mark.parametrize("window", [0, 300])
@pytest.mark.parametrize("kpw", [128, 256])
@pytest.mark.parametrize("H,Hkv", [(32, 8), (8, 8), (16, 8), (16, 2)])
def test_decode_attention2(cuda, H, Hkv, kpw, window):
    """ops.decode_attention2 (pre-rotated q, caches that already hold the new row), test_decode2_gpu's shapes"""
    from videoglamm_amd import ops
    D, max_len = 128, 2048
    assert ops._lib.load().vg_decode_attention2_supported(H, Hkv, D, ops.BF16)
    ws = ops.decode_attention_workspace(H, Hkv, D, max_len, cuda)
    cases = [c for pos in R.decode_positions(max_len, window) + [31, 32, 33, 1000] for c in R.decode_rounds(H, Hkv, D, max_len, pos, window, seed=8)]

    def kernel(c):
        pos_dev = torch.tensor([c["pos_i"]], dtype=torch.int32, device=cuda)
        o = ops.decode_attention2(c["q"].view(1, H * D).to(cuda), c["k_cache"].to(cuda), c["v_cache"].to(cuda), H, Hkv, D, pos_dev, c["scale"], ws,
                                  window=window, keys_per_wg=kpw)
        return o.view(1, 1, H, D).cpu()
    _check(f"decode_attention2 kpw={kpw} {(H, Hkv, D, max_len, window)}", cases, kernel)
    assert int(ws[-Hkv:].view(torch.int32).abs().sum()) == 0


def _slots(c, row0, n_bound, B, cuda, shared_len=1024):
    """a one-row case laid out for the _rows kernels: keys [0, row0) in the shared caches (their later rows hold other values: never read), keys
    [row0, n_bound) in each of B slots"""
    g = torch.Generator().manual_seed(c["pos_i"])
    pk, pv = torch.randn(shared_len, *c["k_cache"].shape[1:], generator=g).to(torch.bfloat16), torch.randn(shared_len, *c["v_cache"].shape[1:], generator=g).to(torch.bfloat16)
    pk[:row0], pv[:row0] = c["k_cache"][:row0], c["v_cache"][:row0]
    ks = c["k_cache"][row0:n_bound][None].repeat(B, 1, 1, 1).contiguous()
    vs = c["v_cache"][row0:n_bound][None].repeat(B, 1, 1, 1).contiguous()
    return pk.to(cuda), pv.to(cuda), ks.to(cuda), vs.to(cuda)


@pytest.mark.parametrize("Ppre", [256, 255, 257, 99])
def test_decode_attention2_rows(cuda, Ppre):
    """ops.decode_attention2_rows (test_qkv_rope_and_attention_rows_bitwise's layout: Llama-3 heads, 256 keys per workgroup, the prefix on, before and
    past a key-block boundary): three rows holding the same step, each against the float64 statement"""
    from videoglamm_amd import ops
    from videoglamm_amd.prompts import slot_layout
    H, Hkv, D, kpw, B = 32, 8, 128, 256, 3
    n_bound = Ppre + 80
    row0, _ = slot_layout(Ppre, kpw, n_bound)
    ws = ops.decode_attention2_rows_workspace(H, Hkv, D, n_bound, kpw, B, cuda)
    cases = [c for pos in (Ppre, Ppre + 1, Ppre + 40, n_bound - 1) for c in R.decode_rounds(H, Hkv, D, n_bound, pos, 0, seed=9)]

    def kernel(c):
        pk, pv, ks, vs = _slots(c, row0, n_bound, B, cuda)
        pos_dev = torch.full((B,), c["pos_i"], dtype=torch.int32, device=cuda)
        q = c["q"].view(1, H * D).repeat(B, 1).contiguous().to(cuda)
        o = ops.decode_attention2_rows(q, pk, pv, ks, vs, row0, H, Hkv, D, pos_dev, n_bound, c["scale"], ws, keys_per_wg=kpw).cpu()
        assert torch.equal(o[0], o[1]) and torch.equal(o[0], o[2])
        return o[1].view(1, 1, H, D)
    _check(f"decode_attention2_rows Ppre={Ppre}", cases, kernel)


@pytest.mark.parametrize("kpw_min", [0, 8192])
@pytest.mark.parametrize("window", [0, 63, 200])
@pytest.mark.parametrize("Ppre", [300, 520, 512])
def test_decode_attention_rows(cuda, Ppre, window, kpw_min):
    """ops.decode_attention_rows (test_attention_rows_bitwise's layout: Phi-3-mini heads; kpw_min = 0: 128 keys per workgroup on every row, 8192: 64)"""
    from videoglamm_amd import ops
    from videoglamm_amd.prompts import slot_layout
    H, Hkv, D, B = 32, 32, 96, 3
    assert ops._lib.load().vg_decode_attention_rows_supported(H, Hkv, D, ops.BF16)
    n_bound = Ppre + 80
    row0, _ = slot_layout(Ppre, 128, n_bound)
    cos, sin = _tables(1024, D)
    g_cos, g_sin = cos.to(cuda), sin.to(cuda)
    ws = ops.decode_attention_rows_workspace(H, Hkv, D, n_bound, B, cuda)
    cases = [_fused(c, cos, sin) for pos in (Ppre, Ppre + 1, Ppre + 40, n_bound - 1) for c in R.decode_rounds(H, Hkv, D, n_bound, pos, window, seed=10)]

    def kernel(c):
        pk, pv, ks, vs = _slots(c, row0, n_bound, B, cuda)
        pos_dev = torch.full((B,), c["pos_i"], dtype=torch.int32, device=cuda)
        o = ops.decode_attention_rows(c["qkv"].repeat(B, 1).contiguous().to(cuda), pk, pv, ks, vs, row0, g_cos, g_sin, H, Hkv, D, pos_dev, n_bound, c["scale"], ws,
                                      window=window, kpw_min=kpw_min).cpu()
        assert torch.equal(o[0], o[1]) and torch.equal(o[0], o[2])
        assert torch.equal(vs[2, c["pos_i"] - row0].cpu(), c["v"][0, c["pos_i"]])
        return o[1].view(1, 1, H, D)
    _check(f"decode_attention_rows Ppre={Ppre} window={window} kpw_min={kpw_min}", cases, kernel)
