"""Per-token scores on the MI355X (vg_scores.hip): vg_token_scores_rows against the CPU statement of its contract
(tests/_scores_ref.py) — top2 and margin exactly, logprob within a tolerance the self-check shows cannot hide a dropped, doubled or mis-picked
entry — its structure (row independence, reused workspace, one slot written), its entry checks, and the scores through the decode step end to
end: generate() eager / graph-replayed / sampled / forced, generate_prompts() and generate_clips() batched against the per-row loops, and the
façade's return_scores."""
import ctypes

import numpy as np
import pytest
import torch

import _scores_ref as R

torch.set_grad_enabled(False)

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 64, 65, 2048, 2049, 32064, 128256]
CAP = 8
SENT_F, SENT_I = 777.0, -7


# ------------------------------------------------------------------ the kernel
def _key(value, idx):
    """the packed (ordered value bits, ~index) key vg_argmax_partial leaves for entry idx of value `value`, as a signed int64"""
    u = int(np.float32(value).view(np.uint32))
    u = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    k = (u << 32) | ((0xFFFFFFFF - idx) & 0xFFFFFFFF)
    return k - (1 << 64) if k >= (1 << 63) else k


def _rows16(n):
    """16 rows of n entries (every |logprob| stays below 32): random (sigma <= 2.5), ties, signs, peaked / two-entry / flat, the crafted rows of the self-check"""
    g = np.random.default_rng(1000 + n)
    rows = [(g.standard_normal(n) * s).astype(np.float32) for s in (2.5, 1.0, 0.3)]
    x = (g.standard_normal(n) * 2).astype(np.float32)
    x[0] = x[n - 1] = 9.0                                            # maxima tied at (0, n - 1)
    rows.append(x)
    x = (g.standard_normal(n) * 2).astype(np.float32)
    a, b = (2047, 2048) if n > 2048 else (n // 2 - 1 if n > 2 else 0, n // 2 if n > 2 else 1)
    x[a] = x[b] = 9.5                                                # ... on both sides of a slice edge
    rows.append(x)
    x = (g.standard_normal(n) * 2).astype(np.float32)
    x[[n - 1, n // 2, 0] if n > 2 else [0, 1]] = 8.0                 # a three-way tie
    rows.append(x)
    rows.append(np.full(n, -1.5, np.float32))                        # all equal
    rows.append((-np.abs(g.standard_normal(n)) * 3 - 0.5).astype(np.float32))      # all negative
    x = (g.standard_normal(n) * 2).astype(np.float32)
    i = 4 * ((n - 2) // 8)
    x[i], x[i + 1] = 11.0, 10.5                                      # the two largest next to each other, in one aligned 16-byte chunk
    rows.append(x)
    x = g.standard_normal(n).astype(np.float32)
    x[n // 3] += 20.0                                                # peaked
    rows.append(x)
    rows.append(R.crafted("two", n)[0] if n > 2 else np.array([0.0, -0.75], np.float32))
    rows.append(R.crafted("flat", n)[0])
    rows.append(R.crafted("slices", n)[0] if n > 2048 else (g.standard_normal(n) * 3).astype(np.float32))
    x = (g.standard_normal(n) * 2).astype(np.float32)
    x[n - 1] = 12.0                                                  # the maximum in the last entry of the last slice
    rows.append(x)
    while len(rows) < 16:
        rows.append((g.standard_normal(n) * 2.5).astype(np.float32))
    return np.stack(rows)


def _launch(cuda, x, picks, form, pad, steps=None, ws=None, cap=CAP):
    """one launch on rows x [B, n] (numpy) -> (scores [B, cap, 2], top2 [B, cap, 2]) on the host.  pad: ldx = n + 24 with NaN in the gap;
    either way NaN guard rows sit before and after the buffer's rows.  Histories are sentinel-filled."""
    from videoglamm_amd import ops
    B, n = x.shape
    ldx = n + (24 if pad else 0)
    buf = torch.full((B + 2, ldx), float("nan"), dtype=torch.float32)
    buf[1:B + 1, :n] = torch.from_numpy(x)
    buf = buf.to(cuda)
    logits = buf[1:B + 1, :n]
    step = torch.tensor([b % cap for b in range(B)] if steps is None else steps, dtype=torch.int32, device=cuda)
    scores = torch.full((B, cap, 2), SENT_F, dtype=torch.float32, device=cuda)
    top2 = torch.full((B, cap, 2), SENT_I, dtype=torch.int64, device=cuda)
    if form == "tok":
        kw = dict(tok=torch.tensor([int(p) for p in picks], dtype=torch.int64, device=cuda))
    else:
        kw = dict(acc=torch.tensor([_key(x[b, p] if 0 <= p < n else 0.0, int(p)) for b, p in enumerate(picks)], dtype=torch.int64, device=cuda))
    ws = ops.token_scores_workspace(B, cuda) if ws is None else ws
    ops.token_scores_rows(logits, step, scores, top2, ws=ws, **kw)
    if "acc" in kw:
        assert kw["acc"].tolist() == [_key(x[b, p] if 0 <= p < n else 0.0, int(p)) for b, p in enumerate(picks)]      # read, not cleared
    return scores.cpu(), top2.cpu(), step.cpu().tolist()


def _check(x, picks, scores, top2, steps, ref, cap=CAP):
    lp, mg, t2 = ref
    B = x.shape[0]
    for b in range(B):
        j = steps[b]
        assert torch.equal(top2[b, j], torch.from_numpy(t2[b])), (b, top2[b, j].tolist(), t2[b].tolist())
        assert torch.equal(scores[b, j, 1], torch.tensor(mg[b])), (b, float(scores[b, j, 1]), float(mg[b]))
        err = abs(float(scores[b, j, 0]) - lp[b])
        assert err <= R.tol(lp[b]), (b, int(picks[b]), float(scores[b, j, 0]), lp[b], err, R.tol(lp[b]))
        other = torch.ones(cap, dtype=torch.bool)
        other[j] = False                                             # nothing but slot step[b] of row b moved
        assert bool((scores[b][other] == SENT_F).all()) and bool((top2[b][other] == SENT_I).all()), b


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_the_contract(cuda, n):
    """top2 / margin exactly and logprob within tol, for the argmax, the argmin and a random pick, B = 16, 5 and 1 on the same rows, ldx = n and
    n + 24, the acc and the tok form; every launch bit-equal to the 16-row launch's rows"""
    x = _rows16(n)
    g = np.random.default_rng(n)
    picksets = {"argmax": x.argmax(1), "argmin": x.argmin(1), "random": g.integers(0, n, 16)}
    from videoglamm_amd import ops
    for kind, picks in picksets.items():
        ref = R.reference(x, picks)
        assert np.all(np.abs(ref[0]) < 32) and np.all(ref[1] >= 0)
        full = {}
        for form in ("tok", "acc"):
            for pad in (False, True):
                sc, t2, steps = _launch(cuda, x, picks, form, pad)
                _check(x, picks, sc, t2, steps, ref)
                full[form, pad] = (sc, t2)
        base = full["tok", False]
        assert all(torch.equal(v[0], base[0]) and torch.equal(v[1], base[1]) for v in full.values())       # acc == tok, ldx = n == n + 24
        # B = 5 and B = 1: the same rows in other launches, on a workspace reused from launch to launch
        for B, form, pad in ((5, "acc", True), (1, "tok", False)):
            ws = ops.token_scores_workspace(B, cuda)
            for r0 in range(0, 16, B):
                r1 = min(16, r0 + B)
                sub = (ref[0][r0:r1], ref[1][r0:r1], ref[2][r0:r1])
                sc, t2, steps = _launch(cuda, x[r0:r1], picks[r0:r1], form, pad, steps=[r % CAP for r in range(r0, r1)], ws=ws[:r1 - r0])
                _check(x[r0:r1], picks[r0:r1], sc, t2, steps, sub)
                for b in range(r1 - r0):
                    j = (r0 + b) % CAP
                    assert torch.equal(sc[b, j], base[0][r0 + b, j]) and torch.equal(t2[b, j], base[1][r0 + b, j]), (B, r0 + b)
            assert int(ws[:, 384].abs().sum()) == 0          # the tickets reset themselves


@pytest.mark.parametrize("n", [65, 2049, 32064])
def test_kernel_structure(cuda, n):
    from videoglamm_amd import ops
    x = _rows16(n)[:5]
    picks = x.argmax(1)
    ref = R.reference(x, picks)
    ws = ops.token_scores_workspace(5, cuda)
    # mixed steps per row, one of them past the capacity and one negative: those rows write nothing
    steps = [3, CAP, 0, -1, CAP - 1]
    a = _launch(cuda, x, picks, "acc", True, steps=steps, ws=ws)
    b = _launch(cuda, x, picks, "acc", True, steps=steps, ws=ws)        # the reused workspace: bit-equal
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for r, j in enumerate(steps):
        if 0 <= j < CAP:
            _check(x[r:r + 1], picks[r:r + 1], a[0][r:r + 1], a[1][r:r + 1], [j], tuple(v[r:r + 1] for v in ref))
        else:
            assert bool((a[0][r] == SENT_F).all()) and bool((a[1][r] == SENT_I).all()), r
    # a pick outside [0, n): NaN, with top2 / margin as ever
    for form in ("tok", "acc"):
        sc, t2, st = _launch(cuda, x, [-1, n, 0, n + 5, n - 1], form, False, ws=ws)
        for r, bad in enumerate((True, True, False, True, False)):
            assert bool(torch.isnan(sc[r, st[r], 0])) == bad, (form, r)
            assert torch.equal(t2[r, st[r]], torch.from_numpy(ref[2][r])) and float(sc[r, st[r], 1]) == float(ref[1][r])


def test_kernel_entry_checks(cuda):
    """every refusal returns VG_ERR_ARG (-1) without a launch: the histories keep their sentinels"""
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    assert lib.vg_token_scores_workspace_ints() == R.WS_INTS
    n, B = 4096, 2
    x = torch.randn(B, n, device=cuda)
    step = torch.zeros(B, dtype=torch.int32, device=cuda)
    acc = torch.zeros(B, dtype=torch.int64, device=cuda)
    tok = torch.zeros(B, dtype=torch.int64, device=cuda)
    scores = torch.full((B, CAP, 2), SENT_F, dtype=torch.float32, device=cuda)
    top2 = torch.full((B, CAP, 2), SENT_I, dtype=torch.int64, device=cuda)
    ws = ops.token_scores_workspace(B, cuda)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(x=x, ldx=n, n=n, B=B, acc=None, tok=tok, step=step, scores=scores, top2=top2, cap=CAP, ws=ws)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vg_token_scores_rows(p(a["x"]), a["ldx"], a["n"], a["B"], p(a["acc"]), p(a["tok"]), p(a["step"]), p(a["scores"]), p(a["top2"]),
                                        a["cap"], p(a["ws"]), st)

    bad = [dict(x=None), dict(scores=None), dict(top2=None), dict(step=None), dict(acc=acc), dict(tok=None), dict(n=1), dict(n=0), dict(B=0),
           dict(B=17), dict(ldx=n - 1), dict(cap=0), dict(cap=-3), dict(ws=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"vg_token_scores_rows" in lib.vg_last_error()
    torch.cuda.synchronize()
    assert bool((scores == SENT_F).all()) and bool((top2 == SENT_I).all())
    # n <= 2048 is one workgroup per row and takes no workspace; the good call goes through
    assert call(n=2048, ldx=n, ws=None) == 0 and call() == 0 and call(acc=acc, tok=None) == 0
    torch.cuda.synchronize()
    assert not bool((scores[:, 0] == SENT_F).any()) and bool((scores[:, 1:] == SENT_F).all())


# ------------------------------------------------------------------ generate(): the single-row decode step
def _setup(cuda, fp8=False):
    import test_sampling_gpu as sg
    return sg._setup(cuda, fp8)


def _gen(P, cfg, ids, n, scores, **kw):
    import test_sampling_gpu as sg
    trace = {"scores": True} if scores else {}
    out, _ = sg._gen(P, cfg, ids, n, trace=trace, **kw)
    return out, trace


def _recompute(dec, P, rows, picks):
    """ops.token_scores_rows applied afterwards to the lm_head of the final-norm rows `rows` that emitted the tokens: the kernel and the bits of
    the step's own launch.  picks: the ids the records should describe -> (scores [G, 2], top2 [G, 2]) on the host"""
    from videoglamm_amd import ops
    G = len(rows)
    sc = torch.zeros(1, G, 2, dtype=torch.float32, device=P.device)
    t2 = torch.zeros(1, G, 2, dtype=torch.int64, device=P.device)
    ws = ops.token_scores_workspace(1, P.device)
    for j, (h, pick) in enumerate(zip(rows, picks)):
        logits = dec.proj.lm_head(False, P, h.reshape(1, -1))
        ops.token_scores_rows(logits.view(1, -1), torch.tensor([j], dtype=torch.int32, device=P.device), sc, t2,
                              tok=torch.tensor([int(pick)], dtype=torch.int64, device=P.device), ws=ws)
    return sc[0].cpu(), t2[0].cpu()


def _records(trace):
    s = trace["scores"]
    assert s["logprob"].dtype == np.float32 and s["margin"].dtype == np.float32 and s["top2"].dtype == np.int64
    return torch.from_numpy(np.stack([s["logprob"], s["margin"]], 1)), torch.from_numpy(s["top2"])


def _same_records(a, b):
    for k in ("logprob", "margin", "top2"):
        assert a["scores"][k].shape == b["scores"][k].shape and np.array_equal(a["scores"][k], b["scores"][k], equal_nan=True), k


@pytest.mark.parametrize("fp8", [False, True])
def test_generate_greedy_records(cuda, monkeypatch, fp8):
    from videoglamm_amd.vlm import LlamaDecoder
    monkeypatch.setenv("VG_DECODE_AHEAD", "0")
    P, cfg, ids, S = _setup(cuda, fp8)
    n = 9
    plain, t0 = _gen(P, cfg, ids, n, False)
    out, t1 = _gen(P, cfg, ids, n, True)
    dec = P._decoder
    assert out == plain and t0["argmax"] == t1["argmax"] == out[S:]
    sc, t2 = _records(t1)
    assert sc.shape == (n, 2) and t2.shape == (n, 2)
    assert t2[:, 0].tolist() == t1["argmax"] and bool((sc[:, 1] >= 0).all()) and bool((sc[:, 0] <= 0).all())
    want = _recompute(dec, P, [dec.hid_all[S - 1 + j] for j in range(n)], t1["argmax"])
    assert torch.equal(sc, want[0]) and torch.equal(t2, want[1])
    assert sorted(map(str, dec.graphs)) == sorted(map(str, [0, (0, "scores")]))          # the step with scores is a graph of its own
    # a second call on the reused decoder; then eager, on a decoder of its own: the same records bit for bit
    out2, t2nd = _gen(P, cfg, ids, n, True)
    assert out2 == out
    _same_records(t2nd, t1)
    P._decoder = LlamaDecoder(P, cfg["llm"], dec.max_len, use_graph=False)
    out3, t3 = _gen(P, cfg, ids, n, True)
    assert out3 == out and not P._decoder.graphs
    _same_records(t3, t1)
    # max_new_tokens = 0 and 1
    _, te = _gen(P, cfg, ids, 0, True)
    assert te["scores"]["logprob"].shape == (0,) and te["scores"]["top2"].shape == (0, 2)
    _, t1only = _gen(P, cfg, ids, 1, True)
    assert np.array_equal(t1only["scores"]["top2"], t1["scores"]["top2"][:1]) and np.array_equal(t1only["scores"]["logprob"], t1["scores"]["logprob"][:1])
    P._decoder = None


@pytest.mark.parametrize("k", [20, 0])
def test_generate_sampled_records(cuda, monkeypatch, k):
    """the fast (k = 20) and the general (k = 0) sampling route: the same ids with and without scores, the record describes the drawn id"""
    monkeypatch.setenv("VG_DECODE_AHEAD", "0")
    P, cfg, ids, S = _setup(cuda)
    n = 8
    s = dict(T=1.5, k=k, p=0.95, seed=11)
    plain, _ = _gen(P, cfg, ids, n, False, sampling=s)
    out, tr = _gen(P, cfg, ids, n, True, sampling=s)
    dec = P._decoder
    assert out == plain and tr["argmax"] == out[S:] and dec.samp_fast == (k == 20)
    sc, t2 = _records(tr)
    rows = [dec.hid_all[S - 1 + j] for j in range(n)]
    want = _recompute(dec, P, rows, tr["argmax"])                    # logprob of the DRAWN id
    assert torch.equal(sc, want[0]) and torch.equal(t2, want[1])
    greedy = _recompute(dec, P, rows, t2[:, 0].tolist())             # top2 / margin: the greedy recomputation's
    assert torch.equal(t2, greedy[1]) and torch.equal(sc[:, 1], greedy[0][:, 1])
    assert t2[:, 0].tolist() != tr["argmax"]                         # (T = 1.5: some draw is not the argmax, so the two picks differ)
    P._decoder = None


@pytest.mark.parametrize("ahead", ["0", "1"])
def test_generate_forced_tokens(cuda, monkeypatch, ahead):
    """teacher forcing (on the host hand-over and on the device table): the records describe the model's own pick, not the forced id"""
    from videoglamm_amd import synth
    monkeypatch.setenv("VG_DECODE_AHEAD", ahead)
    P, cfg, ids, S = _setup(cuda)
    n = 8
    hook = synth.forced_tokens_hook({0: 17, 3: 4242, 4: 99})
    plain, t0 = _gen(P, cfg, ids, n, False, hook=hook)
    out, tr = _gen(P, cfg, ids, n, True, hook=hook)
    assert out == plain and [out[S], out[S + 3], out[S + 4]] == [17, 4242, 99] and tr["argmax"] == t0["argmax"] != out[S:]
    sc, t2 = _records(tr)
    assert t2[:, 0].tolist() == tr["argmax"] and sc.shape == (n, 2)
    dec = P._decoder
    want = _recompute(dec, P, [dec.hid_all[S - 1 + j] for j in range(n)], tr["argmax"])
    assert torch.equal(sc, want[0]) and torch.equal(t2, want[1])
    P._decoder = None


# ------------------------------------------------------------------ batched against the per-row loops
def _llm(cuda, model, dw):
    import test_prompts_batched_gpu as llama
    import test_prompts_batched_phi3_gpu as phi3
    mod = phi3 if model == "phi3" else llama
    P, cfg, tw = mod._llm(cuda)
    if dw:
        cfg = dict(cfg, llm=dict(cfg["llm"], decode_weights=dw))
    return mod, P, cfg, tw


MODELS = [("llama", None), ("llama", "fp8"), ("phi3", None), ("phi3", "fp8")]


def _eos_from(free, lens, B):
    """the rows' own tokens at generated positions 1..5 as EOS ids: the rows stop at different steps"""
    return sorted({int(o[L + 1 + b % 5]) for b, (o, L) in enumerate(zip(free, lens))})


@pytest.mark.parametrize("model,dw", MODELS)
def test_prompts_batched_equals_sequential(cuda, monkeypatch, model, dw):
    mod, P, cfg, tw = _llm(cuda, model, dw)
    B, n = 5, 9
    ids = mod._prompts(B, seed=3)
    lens = [i.numel() for i in ids]
    free, _ = mod._run(P, cfg, tw, ids, n)
    eos = _eos_from(free, lens, B)
    ta, tb = [{"scores": True} for _ in range(B)], [{"scores": True} for _ in range(B)]
    ref, got = None, None
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "0")
    ref = mod._run(P, cfg, tw, ids, n, eos=eos, traces=ta)
    monkeypatch.setenv("VG_PROMPTS_BATCHED", "1")
    got = mod._run(P, cfg, tw, ids, n, eos=eos, traces=tb)
    mod._same(ref, got)
    assert ref[0] == mod._run(P, cfg, tw, ids, n, eos=eos)[0]                       # ... and the ids of a run without scores
    (_, rows), = P._decoder._rows.items()
    assert rows.scores_on is False and sorted(map(str, rows.graphs)) == sorted(map(str, ["greedy", ("greedy", "scores")]))
    G = [len(o) - L for o, L in zip(got[0], lens)]
    assert len(set(G)) > 1
    for b in range(B):
        _same_records(ta[b], tb[b])
        assert tb[b]["scores"]["logprob"].shape == (G[b],) and tb[b]["scores"]["top2"].shape == (G[b], 2)
        assert tb[b]["scores"]["top2"][:, 0].tolist() == tb[b]["argmax"] == got[0][b][lens[b]:]
        assert np.all(tb[b]["scores"]["margin"] >= 0) and np.all(np.isfinite(tb[b]["scores"]["logprob"]))
    assert P._decoder.w8 == (dw == "fp8")


@pytest.mark.parametrize("model,dw", MODELS)
def test_clips_batched_equals_sequential(cuda, monkeypatch, model, dw):
    import test_clips_gpu as cg
    P, cfg = cg._llm(cuda, model, dw)
    B, n = 5, 9
    text, visuals = cg._make(cfg, cuda, B, seed=2, first=1)
    lens = [t[2].numel() for t in text]
    free = [o for o, _ in cg._alone(P, cfg, text, visuals, n)]
    eos = _eos_from(free, lens, B)
    ta, tb = [{"scores": True} for _ in range(B)], [{"scores": True} for _ in range(B)]
    monkeypatch.setenv("VG_CLIPS_BATCHED", "0")
    ref = cg._batched(P, cfg, text, visuals, n, eos=eos, traces=ta)
    monkeypatch.setenv("VG_CLIPS_BATCHED", "1")
    got = cg._batched(P, cfg, text, visuals, n, eos=eos, traces=tb)
    cg._same(got, ref)
    cg._same(got, cg._alone(P, cfg, text, visuals, n, eos=eos))                     # the ids of a run without scores
    rows = cg._rows(P)
    assert ("greedy", "scores") in rows.graphs
    G = [o.numel() - L for (o, _), L in zip(got, lens)]
    assert len(set(G)) > 1
    for b in range(B):
        _same_records(ta[b], tb[b])
        assert tb[b]["scores"]["logprob"].shape == (G[b],)
        assert tb[b]["scores"]["top2"][:, 0].tolist() == tb[b]["argmax"] == got[b][0][lens[b]:].tolist()
    # sampled (the fast route), batched against the loop
    sp = cg._sampling("k20", B)
    sa, sb = [{"scores": True} for _ in range(B)], [{"scores": True} for _ in range(B)]
    monkeypatch.setenv("VG_CLIPS_BATCHED", "0")
    ref = cg._batched(P, cfg, text, visuals, n, samplings=sp, traces=sa)
    monkeypatch.setenv("VG_CLIPS_BATCHED", "1")
    got = cg._batched(P, cfg, text, visuals, n, samplings=sp, traces=sb)
    cg._same(got, ref)
    for b in range(B):
        _same_records(sa[b], sb[b])
        assert sb[b]["argmax"] == got[b][0][lens[b]:].tolist()


# ------------------------------------------------------------------ the façade
def _segs_equal(x, y):
    assert sorted(x) == sorted(y) and all(sorted(x[t]) == sorted(y[t]) for t in x)
    assert all(np.array_equal(x[t][k], y[t][k]) for t in x for k in x[t])


def _is_records(s, G):
    assert sorted(s) == ["logprob", "margin", "top2"] and s["logprob"].shape == (G,) and s["margin"].shape == (G,) and s["top2"].shape == (G, 2)
    assert np.all(s["margin"] >= 0) and np.all(s["logprob"] <= 0)


def test_facade_return_scores(cuda):
    import test_clips_gpu as cg
    m, clips = cg._micro(cuda)
    kw = dict(max_new_tokens=8)
    c = clips[0]
    L = c[3].shape[1]
    ids, segs = m.inference(*c, **kw)
    ids2, segs2, sc = m.inference(*c, return_scores=True, **kw)
    assert torch.equal(ids, ids2) and isinstance(sc, list) and len(sc) == 1
    _segs_equal(segs[0], segs2[0])
    _is_records(sc[0], ids.shape[1] - L)
    # after the boxes and the run-length codes, on the video branch too
    ids3, segs3, boxes, codes, sc3 = m.inference(*c, return_boxes=True, return_rle=True, return_scores=True, use_sam2_video_branch=True, **kw)
    assert torch.equal(ids3, ids) and sorted(boxes[0]) == sorted(segs3[0]) == sorted(codes[0])
    for k in sc[0]:
        assert np.array_equal(sc3[0][k], sc[0][k])
    # inference_prompts: one more list, in prompt order, on the shared route and on the per-prompt calls
    head = c[3][0, :3 + c[0][0].shape[0]]
    g = torch.Generator().manual_seed(9)
    prompts = [torch.cat([head, torch.randint(3, 4000, (4 + 3 * b,), generator=g)])[None] for b in range(3)]
    args = (c[0], c[1], c[2], prompts, c[4], c[5])
    o0, s0 = m.inference_prompts(*args, **kw)
    o1, s1, r1 = m.inference_prompts(*args, return_scores=True, **kw)
    o2, s2, b2, r2 = m.inference_prompts(*args, return_scores=True, return_boxes=True, shared=False, **kw)
    assert len(r1) == len(r2) == 3 and all(torch.equal(a, b) for a, b in zip(o0, o1))
    for b in range(3):
        _segs_equal(s0[b], s1[b])
        _is_records(r1[b], o1[b].shape[1] - prompts[b].shape[1])
        _is_records(r2[b], o2[b].shape[1] - prompts[b].shape[1])
        assert sorted(b2[b]) == sorted(s2[b])
    # inference_clips: one more element in every clip's tuple
    plain = m.inference_clips(clips, **kw)
    got = m.inference_clips(clips, return_scores=True, return_rle=True, **kw)
    for (o, s), (o_, s_, codes_, sc_), cl in zip(plain, got, clips):
        assert torch.equal(o, o_) and len(sc_) == 1 and sorted(codes_[0]) == sorted(s_[0])
        _segs_equal(s[0], s_[0])
        _is_records(sc_[0], o.shape[1] - cl[3].shape[1])
    (_, rows), = m.P._decoder._rows.items()
    assert any(isinstance(k, tuple) and k[-1] == "scores" for k in rows.graphs)
