"""Plain-torch side of the attention accuracy tests (no device code, no GPU import).

* attention64: the statement of _cpu_ops.attention (GQA, causal diagonal shifted by Skv - Sq, window = own position and the window - 1 before it)
  in float64 on the bf16-rounded operands, chunked over query rows; returns the output and the per-row log-sum-exp (the softmax mass of any
  key follows from it: exp(scale * q.k - lse)).
* attention_bf16_model: the HONEST bf16 flash kernel — scores and softmax in fp32, exp(s - m) rounded to bf16 before P.V, fp32 accumulation,
  division by the fp32 row sum, output rounded to bf16.  Its error is what a correct kernel is entitled to.  Its keyword hooks (vis_edit,
  scale_mul, dup_key, split, kv_of_head) exist for the self-check only: they turn it into the wrong kernels the tests must catch.
* row_err: per (batch, query row, head) ||got - ref||_2 / ||ref||_2 over the head dim.
* build_case / decode_rounds: random q/k/v plus probe rows, in which single keys carry most of a row's softmax mass (see build_case).

K_BOUND: a kernel passes a case when max row_err(kernel) <= K_BOUND * max row_err(model) on the same inputs (model evaluated on the CPU inside
the test, never derived from the kernel).  See tests/test_attention_accuracy_gpu.py for the measured kernel / model ratios behind the constant.
"""
import math

import torch

K_BOUND = 4.0
BIG_V = 8.0
MASS_MIN = 0.5


def _visible(i0, i1, Sq, Skv, causal, window):
    """bool [i1 - i0, Skv]: the keys query rows i0 .. i1 - 1 (of Sq) may see"""
    vis = torch.ones(i1 - i0, Skv, dtype=torch.bool)
    if causal:
        d = torch.arange(i0, i1)[:, None] + (Skv - Sq)
        j = torch.arange(Skv)[None, :]
        vis &= j <= d
        if window:
            vis &= j > d - window
    else:
        assert not window, "a sliding window needs the causal mask"
    return vis


def _heads(q, k, v, b, dtype, kv_of_head=None):
    Hq, Hkv = q.shape[2], k.shape[2]
    idx = torch.arange(Hq) // (Hq // Hkv) if kv_of_head is None else torch.as_tensor(kv_of_head)
    return k[b].to(dtype).permute(1, 0, 2)[idx], v[b].to(dtype).permute(1, 0, 2)[idx]      # [Hq, Skv, D], [Hq, Skv, DV]


def attention64(q, k, v, scale, causal=False, window=0, row0=0, Sq_total=None, chunk=512):
    """q [B, n, Hq, D] (rows row0 .. row0 + n - 1 of a sequence of Sq_total queries), k [B, Skv, Hkv, D], v [B, Skv, Hkv, DV]
    -> (out float64 [B, n, Hq, DV], lse float64 [B, n, Hq])"""
    B, n, Hq, _ = q.shape
    Skv, DV = k.shape[1], v.shape[3]
    Sq = Sq_total if Sq_total is not None else n
    out = torch.empty(B, n, Hq, DV, dtype=torch.float64)
    lse = torch.empty(B, n, Hq, dtype=torch.float64)
    for b in range(B):
        kf, vf = _heads(q, k, v, b, torch.float64)
        for i0 in range(0, n, chunk):
            i1 = min(n, i0 + chunk)
            s = (q[b, i0:i1].double().permute(1, 0, 2) @ kf.transpose(1, 2)) * scale                  # [Hq, rows, Skv]
            s.masked_fill_(~_visible(row0 + i0, row0 + i1, Sq, Skv, causal, window)[None], float("-inf"))
            l = torch.logsumexp(s, dim=-1, keepdim=True)
            out[b, i0:i1] = (torch.exp(s - l) @ vf).permute(1, 0, 2)
            lse[b, i0:i1] = l[..., 0].t()
    return out, lse


def attention_bf16_model(q, k, v, scale, causal=False, window=0, row0=0, Sq_total=None, chunk=512,
                         vis_edit=None, scale_mul=1.0, dup_key=None, split=None, kv_of_head=None):
    """The honest bf16 flash kernel (module docstring) -> bf16 [B, n, Hq, DV].  Self-check hooks: vis_edit(vis, i0, i1) edits the visibility of
    absolute rows i0 .. i1 - 1 in place; scale_mul multiplies the softmax scale; dup_key counts one key twice; split = (boundary, kind) merges
    the keys below / from `boundary` as two partial softmaxes — kind "ok" (max / sum weights), "equal" (mean of the two normalised partials),
    "norescale" (partials added without bringing them to a common maximum); kv_of_head maps query heads to KV heads."""
    B, n, Hq, _ = q.shape
    Skv, DV = k.shape[1], v.shape[3]
    Sq = Sq_total if Sq_total is not None else n
    out = torch.empty(B, n, Hq, DV, dtype=torch.bfloat16)
    spans = [(0, Skv)] if split is None else [(0, split[0]), (split[0], Skv)]
    for b in range(B):
        kf, vf = _heads(q, k, v, b, torch.float32, kv_of_head)
        for i0 in range(0, n, chunk):
            i1 = min(n, i0 + chunk)
            s = (q[b, i0:i1].float().permute(1, 0, 2) @ kf.transpose(1, 2)) * (scale * scale_mul)
            vis = _visible(row0 + i0, row0 + i1, Sq, Skv, causal, window)
            if vis_edit is not None:
                vis_edit(vis, row0 + i0, row0 + i1)
            s.masked_fill_(~vis[None], float("-inf"))
            parts = []
            for j0, j1 in spans:
                sj = s[..., j0:j1]
                m = sj.amax(dim=-1, keepdim=True)
                m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))      # a span with no visible key: weight 0
                p = torch.exp(sj - m)
                if dup_key is not None and j0 <= dup_key < j1:
                    p[..., dup_key - j0] *= 2.0
                parts.append((m, p.sum(-1, keepdim=True), p.to(torch.bfloat16).float() @ vf[:, j0:j1]))
            if len(parts) == 1:
                o = parts[0][2] / parts[0][1]
            elif split[1] == "equal":
                o = 0.5 * (parts[0][2] / parts[0][1].clamp_min(1e-30) + parts[1][2] / parts[1][1].clamp_min(1e-30))
            elif split[1] == "norescale":
                o = (parts[0][2] + parts[1][2]) / (parts[0][1] + parts[1][1])
            else:
                m = torch.maximum(parts[0][0], parts[1][0])
                w0, w1 = torch.exp(parts[0][0] - m), torch.exp(parts[1][0] - m)
                o = (parts[0][2] * w0 + parts[1][2] * w1) / (parts[0][1] * w0 + parts[1][1] * w1)
            out[b, i0:i1] = o.permute(1, 0, 2).to(torch.bfloat16)
    return out


def row_err(got, ref64):
    """[B, n, H]: ||got - ref||_2 / ||ref||_2 over the head dim"""
    return (got.double() - ref64).norm(dim=-1) / ref64.norm(dim=-1).clamp_min(1e-300)


def passes(err_kernel, err_model, k=K_BOUND):
    """the bound of the module docstring; a non-finite error fails"""
    return bool(torch.isfinite(err_kernel).all()) and float(err_kernel.max()) <= k * float(err_model.max())


# ------------------------------------------------------------------ inputs in which every probed key matters
def probe_keys(Skv, split_edges=()):
    """key positions to probe, most important first: the ends, both sides of every split-KV boundary, of every 256-, 128-, 64-key boundary"""
    T = [0, 1, Skv - 2, Skv - 1]
    for e in split_edges:
        T += [e - 1, e]
    for step in (256, 128, 64):
        for e in range(step, Skv, step):
            T += [e - 1, e]
    seen, out = set(), []
    for t in T:
        if 0 <= t < Skv and t not in seen:
            seen.add(t)
            out.append(t)
    return out


def build_case(B, Hq, Hkv, Sq, Skv, D, DV=None, causal=False, window=0, seed=0, split_edges=(), rows=None, batches=None, groups=None,
               rnd=0, frac=0.25):
    """Random bf16 q [B, Sq, Hq, D], k [B, Skv, Hkv, D], v [B, Skv, Hkv, DV] plus probes.

    A positive probe (b, g, i, t) makes key t of KV head g carry most of the softmax mass of query row i (all query heads of group g, which share
    one q vector on that row): k[t] = c q[i] with c such that the logit is ln(visible keys) + 2.5, and v[t] gets +8 in channel t mod DV.  A kernel
    that drops, doubles or mis-weights key t gets row i wrong by O(1).  Every key of probe_keys() is probed from its own (batch, KV head, row);
    causal cases also probe each tile-edge row's (i = -1, 0 mod 64) own diagonal key, windowed cases the oldest visible key of the rows
    i = 1, 62 (mod 64) and of the rows whose oldest key sits on a 64-key boundary.
    A negative probe (b, g, i, t) puts c q[i] (logit + 2) and the large value on a key row i must NOT see: diag + 1 and diag - window of the same
    tile-edge / window rows.  A kernel that leaks it gets row i wrong by O(1); a correct kernel never notices.
    A key claimed by several probes holds the sum of their c q[i] (random q are near orthogonal); check_probes() asserts what came of it.

    At most `frac` of the (batch, KV head, row) triples inside rows / batches / groups (the part of the output the caller checks) carry a positive
    probe; what does not fit goes to later rounds: call again with rnd = 1 .. n_rounds - 1.  One-row cases (Sq == 1: a decode step) hold one probe
    per call in at most half of their KV heads (at least one)."""
    DV = DV or D
    g = torch.Generator().manual_seed(1000 * seed + Sq + Skv + D)
    q = torch.randn(B, Sq, Hq, D, generator=g).to(torch.bfloat16)
    k = torch.randn(B, Skv, Hkv, D, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Skv, Hkv, DV, generator=g).to(torch.bfloat16)
    r0, r1 = rows or (0, Sq)
    planes = [(b, h) for b in (batches if batches is not None else range(B)) for h in (groups if groups is not None else range(Hkv))]
    G, off, scale = Hq // Hkv, Skv - Sq, D ** -0.5
    diag = lambda i: i + off if causal else Skv - 1                                    # noqa: E731
    lo_key = lambda i: max(0, diag(i) - window + 1) if window else 0                   # noqa: E731

    reserved, free_targets = [], []                     # reserved: (i, t) probed in EVERY plane; free_targets: t, any row that sees it
    if causal and Sq > 1:
        for i in range(r0, r1):
            if i % 64 in (63, 0):
                reserved.append((i, diag(i)))
            elif window and diag(i) - window + 1 >= 0 and (i % 64 in (1, 62) or (diag(i) - window + 1) % 64 in (0, 63)):
                reserved.append((i, diag(i) - window + 1))
    free_targets = probe_keys(Skv, split_edges)
    if causal and Sq == 1:
        free_targets = [Skv - 1, Skv - 2] + ([lo_key(0)] if window else []) + free_targets
        free_targets = list(dict.fromkeys(t for t in free_targets if lo_key(0) <= t < Skv))
    elif causal and window:
        free_targets = [t for t in free_targets if t - off + window - 1 >= r0]          # keys some checked row can see
    taken = {t for _, t in reserved}                     # (a 64-key boundary key that is a tile-edge row's diagonal key is probed there)
    free_targets = [t for t in free_targets if t not in taken]
    total = len(planes) * (r1 - r0)
    budget = max(1, len(planes) // 2) if Sq == 1 else int(frac * total)
    cap = budget - len(reserved) * len(planes)
    assert cap >= 1, "no room for probes beside the tile-edge rows"
    n_rounds = max(1, -(-len(free_targets) // cap))
    mine = free_targets[rnd * cap:(rnd + 1) * cap]

    used = {p: {i for i, _ in reserved} for p in planes}
    pos, neg = [], []
    for p in planes:
        pos += [(p[0], p[1], i, t) for i, t in reserved]
    nxt = 0
    for t in mine:
        lo, hi = (max(r0, t - off), r1 - 1) if causal else (r0, r1 - 1)
        if causal and window:
            hi = min(hi, t - off + window - 1)
        if hi < lo:          # no checked row sees this key
            continue
        placed = False
        for tries in range(len(planes)):
            p = planes[(nxt + tries) % len(planes)]
            start = lo + int(torch.randint(0, hi - lo + 1, (1,), generator=g))
            for s in range(hi - lo + 1):
                i = lo + (start - lo + s) % (hi - lo + 1)
                if i not in used[p]:
                    used[p].add(i)
                    pos.append((p[0], p[1], i, t))
                    placed = True
                    break
            if placed:
                nxt = (nxt + tries + 1) % len(planes)
                break
        assert placed, f"no free row sees key {t}"
    if causal:          # the keys just outside the mask of the tile-edge / window rows (a one-row case: of its only row, in every KV head)
        neg_rows = [(p[0], p[1], 0) for p in planes] if Sq == 1 else [(p[0], p[1], i) for p in planes for i, _ in reserved]
        for b, h, i in neg_rows:
            if diag(i) + 1 < Skv:
                neg.append((b, h, i, diag(i) + 1))
            if window and diag(i) - window >= 0:
                neg.append((b, h, i, diag(i) - window))

    # write the probes: q of a probe row is shared by its group's heads; probed keys start from zero and collect c q[i]
    kf = k.float()
    for b, h, i, _ in pos + neg:
        q[b, i, h * G:(h + 1) * G] = q[b, i, h * G]
    # rows that claim a common key (a tile-edge row's diagonal key is its neighbour's diag + 1): each row's q is made orthogonal to the earlier
    # rows it shares a key with, so that one row's c q[i] adds nothing to the other's logit
    claims, share = {}, {}
    for b, h, i, t in pos + neg:
        claims.setdefault((b, h, t), set()).add(i)
    for (b, h, t), rs in claims.items():
        for i in rs:
            share.setdefault((b, h, i), set()).update(j for j in rs if j < i)
    for (b, h, i) in sorted(share):
        if share[(b, h, i)]:
            Q = torch.stack([q[b, j, h * G].double() for j in sorted(share[(b, h, i)])], dim=1)
            x = q[b, i, h * G].double()
            q[b, i, h * G:(h + 1) * G] = (x - Q @ torch.linalg.lstsq(Q, x[:, None]).solution[:, 0]).to(torch.bfloat16)
    for b, h, t in {(b, h, t) for b, h, _, t in pos + neg}:
        kf[b, t, h] = 0
        v[b, t, h, t % DV] += BIG_V
    for lst, extra in ((pos, 0.0), (neg, 2.0)):
        for b, h, i, t in lst:
            qi = q[b, i, h * G].float()
            n_vis = diag(i) - lo_key(i) + 1
            L = min(math.log(n_vis) + 2.5 + extra, 28.0)
            kf[b, t, h] += qi * (L / (scale * float(qi @ qi)))
    k = kf.to(torch.bfloat16)
    return dict(q=q, k=k, v=v, scale=scale, causal=causal, window=window, pos=pos, neg=neg, n_rounds=n_rounds, rows=(r0, r1),
                batches=list(batches) if batches is not None else list(range(B)), groups=list(groups) if groups is not None else list(range(Hkv)))


def checked(case, out):
    """the part of an output [B, Sq, Hq, DV] the case checks: its batches, rows and the query heads of its KV groups"""
    G = case["q"].shape[2] // case["k"].shape[2]
    heads = [h * G + j for h in case["groups"] for j in range(G)]
    return out[case["batches"]][:, case["rows"][0]:case["rows"][1]][:, :, heads]


def reference(case, model=attention_bf16_model, **kw):
    """(ref64, lse) or the model's output on the checked part of a case"""
    q = checked(case, case["q"])
    k, v = case["k"][case["batches"]][:, :, case["groups"]], case["v"][case["batches"]][:, :, case["groups"]]
    return model(q, k, v, case["scale"], case["causal"], case["window"], row0=case["rows"][0], Sq_total=case["q"].shape[1], **kw)


def check_probes(case, lse):
    """CPU assertions on the inputs themselves: every positive probe holds >= MASS_MIN of its row's softmax mass (all heads of the group); every
    negative probe would outweigh the whole row (weight >= 1 relative to the row's sum) if it leaked; at most 25 % of the checked rows are
    probe rows (one-row cases: see build_case)."""
    q, k, G = case["q"], case["k"], case["q"].shape[2] // case["k"].shape[2]
    bi, gi, r0 = {b: n for n, b in enumerate(case["batches"])}, {h: n for n, h in enumerate(case["groups"])}, case["rows"][0]
    for lst, least in ((case["pos"], MASS_MIN), (case["neg"], 1.0)):
        for b, h, i, t in lst:
            for j in range(G):
                s = float(q[b, i, h * G + j].double() @ k[b, t, h].double()) * case["scale"]
                w = math.exp(s - float(lse[bi[b], i - r0, gi[h] * G + j]))
                assert w >= least, (b, h, i, t, w)
    n_rows = len(case["batches"]) * len(case["groups"]) * (case["rows"][1] - case["rows"][0])
    if q.shape[1] > 1:
        assert len({(b, h, i) for b, h, i, _ in case["pos"]}) <= 0.25 * n_rows
    assert len(case["pos"]) > 0


def evaluate(cases, kernel):
    """cases: the rounds of one case; kernel(case) -> the checked part of the output (checked()).  -> (max row error of the kernel, of the model),
    after asserting the probe conditions on the CPU."""
    ek, em = [], []
    for case in cases:
        ref, lse = reference(case, attention64)
        check_probes(case, lse)
        em.append(row_err(reference(case), ref).max())
        ek.append(row_err(kernel(case), ref).max())
    return torch.stack(ek), torch.stack(em)


def all_rounds(*args, **kw):
    first = build_case(*args, **kw)
    return [first] + [build_case(*args, rnd=r, **kw) for r in range(1, first["n_rounds"])]


# ------------------------------------------------------------------ decode steps: one query row against a cache
def rope_rows(x, cos, sin, pos):
    """x [H, D] bf16 rotated at position pos (half-split pairs), fp32 arithmetic on the fp32 tables, rounded to bf16 once"""
    D = x.shape[-1]
    c, s, xf = cos[pos].float(), sin[pos].float(), x.float()
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(torch.bfloat16)


def decode_positions(max_len, window=0):
    """positions on both sides of every 64- / 128- / 256-key block boundary family, the ends, and (windowed) around the window's length"""
    P = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, max_len // 2 + 5, max_len - 1]
    if window:
        P += [window - 1, window, window + 1, window + 63, window + 64]
    return sorted({p for p in P if 0 <= p < max_len})


def decode_rounds(H, Hkv, D, max_len, pos, window=0, seed=0):
    """the rounds of a one-row case at position pos (keys 0 .. pos valid), each with caches of max_len rows: rows past pos hold what an earlier,
    longer sequence left (random), and the first of them the negative probe diag + 1.  -> dicts of build_case() plus k_cache / v_cache
    [max_len, Hkv, D] (the valid rows are k[0] / v[0])."""
    out = []
    for case in all_rounds(1, H, Hkv, 1, pos + 1, D, causal=True, window=window, seed=seed + pos):
        g = torch.Generator().manual_seed(seed + 7 * pos + 1)
        kc = torch.randn(max_len, Hkv, D, generator=g).to(torch.bfloat16)
        vc = torch.randn(max_len, Hkv, D, generator=g).to(torch.bfloat16)
        kc[: pos + 1], vc[: pos + 1] = case["k"][0], case["v"][0]
        if pos + 1 < max_len:          # the first masked key: aligned with each head group's query, large value
            G = H // Hkv
            for h in range(Hkv):
                qi = case["q"][0, 0, h * G].float()
                kc[pos + 1, h] = (qi * ((math.log(pos + 1) + 4.5) / (case["scale"] * float(qi @ qi)))).to(torch.bfloat16)
                vc[pos + 1, h, (pos + 1) % D] += BIG_V
        case["k_cache"], case["v_cache"], case["pos_i"] = kc, vc, pos
        out.append(case)
    return out
