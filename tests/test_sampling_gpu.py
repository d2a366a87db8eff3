"""Sampled decoding on the MI355X (vg_sample.hip): the kernel against the CPU statement of the contract (tests/_cpu_sampling.py), the device
Philox, the draw's distribution, and the decode loop end to end (eager / graph-replayed / run-ahead / fp8 lm_head, [SEG] rows, no re-capture)."""
import numpy as np
import pytest
import torch

import _cpu_sampling as S

pytestmark = pytest.mark.gpu


def _row(V, seed, ties=0, block=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(V, generator=g) * 2.5
    if ties:
        top = torch.topk(x, 30).values
        at = torch.arange(1000, 1000 + ties) if block else torch.randperm(V, generator=g)[:ties]
        x[at] = float(top[-1]) - 0.25      # `ties` equal values just below the 30th largest (block: all in the first fast-route slice)
    return x


def _token(acc):
    return 0xFFFFFFFF - (int(acc[0]) & 0xFFFFFFFF)


@pytest.mark.parametrize("V", [32064, 128256])
def test_kernel_against_the_contract(cuda, V):
    from videoglamm_amd import ops
    rows, skipped, checked = [], 0, 0
    i = 0
    for T in (0.3, 0.6, 1.0, 1.7):
        for k in (0, 1, 5, 50, 64, 65, 1000, V + 7):
            for p in (0.1, 0.9, 1.0):
                rows.append((_row(V, 100 + i), T, k, p))
                i += 1
    for j, k in enumerate((50, 64, 65, 100)):              # 70+ ties at the k-th value
        rows.append((_row(V, 900 + j, ties=80), 1.0, k, 1.0))
        rows.append((_row(V, 950 + j, ties=80), 0.6, k, 0.9))
    n_plain = len(rows)
    for j, k in enumerate((40, 50, 64)):                    # tie overflow of the fast route: 90 ties inside ONE workgroup's slice
        rows.append((_row(V, 970 + j, ties=90, block=True), 1.0, k, 1.0))
        rows.append((_row(V, 980 + j, ties=90, block=True), 1.7, k, 1.0))
    one = torch.full((V,), -float("inf"))
    one[V // 3] = 1.5
    rows += [(one, 1.0, 50, 0.9), (one, 0.6, 0, 1.0)]
    params = torch.zeros(6, dtype=torch.int32, device=cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    acc = torch.zeros(1, dtype=torch.int64, device=cuda)
    u_dev = torch.zeros(1, dtype=torch.float32, device=cuda)
    tok = torch.zeros(1, dtype=torch.int64, device=cuda)
    ws = ops.sample_workspace(cuda)
    fast_checked = 0
    for r, (x, T, k, p) in enumerate(rows):
        xd = x.to(cuda)
        ops.sampling_params(T, k, p, 0, cuda, out=params)
        order, prob, margin = S.kept(x.numpy(), T, k, p)
        # a top-p cut within 1e-6 of 1 - p: the kept set is either side's; the survivors are not compared, a draw only where both sides agree
        sides = [S.kept(x.numpy(), T, k, p + d)[:2] for d in (-1e-6, 1e-6)] if margin < 1e-6 else [(order, prob)]
        if margin < 1e-6:
            skipped += 1
        else:
            idx, pr = ops.sample_survivors(xd, params)
            assert idx.tolist() == sorted(order.tolist()), (r, T, k, p, len(idx), len(order))
            want = dict(zip(order.tolist(), prob.tolist()))
            assert max(abs(float(q) - want[int(j)]) for j, q in zip(idx, pr)) < 1e-6, (r, T, k, p)
            checked += 1
        # overflow rows also draw near the top of the CDF: the last tied entries by index are the ones a slice had to drop
        for u in (0.0, *np.random.default_rng(r).random(2).tolist(), *((0.995, 0.9995) if r >= n_plain else ())):
            draws = [S.draw(o, q, u) for o, q in sides]
            wtok, edge = draws[0][0], min(e for _, e in draws)
            if (edge < 1e-6 and u > 0) or any(t != wtok for t, _ in draws):
                skipped += 1
                continue
            u_dev.fill_(u)
            acc.zero_()
            ops.sample_partial(xd, params, step, acc=acc, tok=tok, u_override=u_dev)
            assert _token(acc) == int(tok[0]) == wtok, (r, T, k, p, u, _token(acc), wtok)
            checked += 1
            # the fast route (it covers 1 <= k <= 64; any other k must fall back inside the launch): the same token and the same key
            if k <= V:
                acc.zero_()
                tok.fill_(-1)
                ops.sample_partial(xd, params, step, acc=acc, tok=tok, u_override=u_dev, fast_ws=ws)
                assert _token(acc) == int(tok[0]) == wtok, ("fast", r, T, k, p, u, _token(acc), wtok)
                fast_checked += ops.sample_fast_route(k, V)
    assert int(ws[-64]) == 0                       # the ticket reset itself after every launch
    assert fast_checked > 150 and skipped < 0.01 * (checked + skipped), (skipped, checked, fast_checked)


def test_device_philox_equals_numpy(cuda):
    from videoglamm_amd import ops
    rng = np.random.default_rng(0)
    seeds = rng.integers(0, 2 ** 63, 10000, dtype=np.int64)
    seeds[:5] = [0, 1, 2 ** 32, 2 ** 63 - 1, 12345]
    steps = rng.integers(0, 4096, 10000).astype(np.int32)
    got = ops.philox(torch.from_numpy(seeds).to(cuda), torch.from_numpy(steps).to(cuda)).cpu().numpy().view(np.uint32)
    want = S.philox_x0(seeds.astype(np.uint64), steps.astype(np.uint64))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("route", ["fast", "general"])
def test_draw_distribution_chi_square(cuda, route):
    """20 000 Philox draws (steps 0..19 999, fixed seed) from one row against the contract's probabilities"""
    from scipy.stats import chisquare
    from videoglamm_amd import ops
    V, N = 32064, 20000
    x = _row(V, 7) * (1.0 if route == "fast" else 1.6)
    T, k, p = (0.6, 50, 0.9) if route == "fast" else (1.0, 0, 0.9)
    order, prob, _ = S.kept(x.numpy(), T, k, p)      # k = 0 over V > 4096 survivors: the row route (every pass reads the row)
    params = ops.sampling_params(T, k, p, 0x5EED_1234_ABCD, cuda)
    steps = torch.arange(N, dtype=torch.int32, device=cuda)
    out = torch.zeros(N, dtype=torch.int64, device=cuda)
    xd = x.to(cuda)
    ws = ops.sample_workspace(cuda) if route == "fast" else None
    for i in range(N):
        ops.sample_partial(xd, params, steps[i:i + 1], tok=out[i:i + 1], fast_ws=ws)
    got = out.cpu().numpy()
    pos = {int(j): n for n, j in enumerate(order)}
    assert all(int(t) in pos for t in got)
    counts = np.bincount([pos[int(t)] for t in got], minlength=len(order)).astype(np.float64)
    exp = prob * N
    big = exp >= 5
    obs = np.concatenate([counts[big], [counts[~big].sum()]]) if (~big).any() else counts[big]
    ex = np.concatenate([exp[big], [exp[~big].sum()]]) if (~big).any() else exp[big]
    pv = chisquare(obs, ex * obs.sum() / ex.sum()).pvalue
    assert pv > 1e-4, pv
    # deterministic: the same seed and steps give the same ids
    again = torch.zeros(N, dtype=torch.int64, device=cuda)
    for i in range(0, N, 997):
        ops.sample_partial(xd, params, steps[i:i + 1], tok=again[i:i + 1])        # the general route draws the same ids as the fast one
    assert torch.equal(again[::997], out[::997])


def _setup(cuda, fp8=False):
    from test_decode2_gpu import _llama2, rnd
    from videoglamm_amd.params import Params
    S_ = 40
    c, sd, x = _llama2(S_)
    if fp8:
        c = dict(c, decode_weights="fp8")
    sd = dict(sd)
    sd["model.text_hidden_fcs.0.0.weight"] = rnd(4096, 4096, dtype=torch.bfloat16, seed=1, scale=0.02)
    sd["model.text_hidden_fcs.0.0.bias"] = rnd(4096, dtype=torch.bfloat16, seed=2, scale=0.02)
    sd["model.text_hidden_fcs.0.2.weight"] = rnd(256, 4096, dtype=torch.bfloat16, seed=3, scale=0.02)
    sd["model.text_hidden_fcs.0.2.bias"] = rnd(256, dtype=torch.bfloat16, seed=4, scale=0.02)
    P = Params(sd, cuda, torch.bfloat16)
    ids = torch.randint(0, 8000, (S_,), generator=torch.Generator().manual_seed(5))
    return P, dict(llm=c, seg_token_idx=8191), ids, S_


def _gen(P, cfg, ids, n, sampling=None, hook=None, trace=None):
    from videoglamm_amd import vlm
    out, emb = vlm.generate(P, cfg, None, None, None, ids, n, visual=torch.empty(0, 4096, dtype=torch.bfloat16, device=P.device),
                            token_hook=hook, trace=trace, sampling=sampling)
    return out.tolist(), emb


def test_generate_sampled_end_to_end(cuda, monkeypatch):
    from videoglamm_amd import synth
    from videoglamm_amd.vlm import LlamaDecoder
    P, cfg, ids, S_ = _setup(cuda)
    n = 12
    monkeypatch.setenv("VG_DECODE_AHEAD", "0")
    greedy = _gen(P, cfg, ids, n)[0]
    # top_k = 1 sampling is greedy
    assert _gen(P, cfg, ids, n, dict(T=0.7, k=1, p=1.0, seed=3))[0] == greedy
    # high entropy (flat T, no top-k / top-p): different seeds draw different ids, the same seed the same ones
    hot = dict(T=50.0, k=0, p=1.0)
    a = _gen(P, cfg, ids, n, dict(hot, seed=1))[0]
    b = _gen(P, cfg, ids, n, dict(hot, seed=2))[0]
    assert a != b and a[S_:] != greedy[S_:]
    assert _gen(P, cfg, ids, n, dict(hot, seed=1))[0] == a
    # the same seed: graph-replayed (above) == eager == run-ahead
    s = dict(T=1.3, k=50, p=0.95, seed=77)
    graphed = _gen(P, cfg, ids, n, s)[0]
    monkeypatch.setenv("VG_DECODE_AHEAD", "1")
    assert _gen(P, cfg, ids, n, s)[0] == graphed
    monkeypatch.setenv("VG_DECODE_AHEAD", "0")
    P._decoder = LlamaDecoder(P, cfg["llm"], P._decoder.max_len, use_graph=False)
    assert _gen(P, cfg, ids, n, s)[0] == graphed
    P._decoder = None
    # [SEG] rows follow the sampled tokens: make the 3rd and 7th sampled ids the [SEG] id, then a greedy run teacher-forced with the sampled
    # ids gives bit-identical embeddings
    seg_cfg = dict(cfg, seg_token_idx=graphed[S_ + 2])
    sampled, emb_s = _gen(P, seg_cfg, ids, n, s)
    assert sampled == graphed and emb_s.shape[0] >= 1
    forced, emb_f = _gen(P, seg_cfg, ids, n, hook=synth.forced_tokens_hook({j: t for j, t in enumerate(sampled[S_:])}))
    assert forced == sampled and torch.equal(emb_s, emb_f)


def test_generate_sampled_fp8_lm_head(cuda, monkeypatch):
    P, cfg, ids, S_ = _setup(cuda, fp8=True)
    s = dict(T=1.3, k=50, p=0.95, seed=77)
    monkeypatch.setenv("VG_DECODE_AHEAD", "0")
    a = _gen(P, cfg, ids, 10, s)[0]
    assert P._decoder.w8
    monkeypatch.setenv("VG_DECODE_AHEAD", "1")
    assert _gen(P, cfg, ids, 10, s)[0] == a
    assert _gen(P, cfg, ids, 10, dict(s, k=1))[0] == _gen(P, cfg, ids, 10)[0]


def test_new_parameters_do_not_recapture(cuda, monkeypatch):
    monkeypatch.setenv("VG_DECODE_AHEAD", "0")
    P, cfg, ids, S_ = _setup(cuda)
    _gen(P, cfg, ids, 6)
    dec = P._decoder
    assert len(dec.graphs) == 1
    outs = set()
    # one graph per route (greedy, fast k <= 64, general), whatever T / k / p / seed
    runs = [(dict(T=1.0, k=50, p=1.0, seed=1), 2), (dict(T=40.0, k=20, p=0.9, seed=5), 2), (dict(T=40.0, k=0, p=0.9, seed=1), 3),
            (dict(T=40.0, k=0, p=0.9, seed=2), 3), (dict(T=40.0, k=3000, p=0.5, seed=9), 3), (dict(T=3.0, k=64, p=1.0, seed=9), 3)]
    for s, n_graphs in runs:
        outs.add(tuple(_gen(P, cfg, ids, 6, s)[0]))
        assert P._decoder is dec and len(dec.graphs) == n_graphs, (s, list(dec.graphs))
    assert len(outs) >= 4
    _gen(P, cfg, ids, 6)
    assert len(dec.graphs) == 3
