"""The CPU statement of vg_token_scores_rows' contract (include/vg_kernels.h): top1 / top2 and the margin in exact fp32, the
log-probability in float64.  Not collected.  Also the twin CPU tests put in place of ops.token_scores_rows / ops.token_scores_workspace
(tests/_cpu_ops.py states the older kernels and stays as it is)."""
import numpy as np
import torch

WS_INTS = 400      # vg_token_scores_workspace_ints(): the twin's workspace has the kernel's size, and stays zero


def tol(ref):
    """|logprob error| allowed against the float64 reference: 2e-6 + 2^-21 * max(1, |ref|).  expf within 2 ulp is 2.4e-7 relative on the mass,
    the fixed-point truncation < 1.2e-7 of the total for n <= 2^17, logf and two fp32 subtractions a few ulp at magnitude <= 32: the bound
    leaves about 2x over their sum."""
    return 2e-6 + 2.0 ** -21 * np.maximum(1.0, np.abs(ref))


def top2_row(x, skip=None):
    """(top1, top2) of one fp32 row: the largest and second-largest entry, ties to the lower index; skip: an index the search does not see
    (the self-check's "dropped entry" mutation)"""
    x = np.asarray(x, dtype=np.float32)
    ok = np.ones(x.shape[0], dtype=bool)
    if skip is not None:
        ok[skip] = False
    idx = np.flatnonzero(ok)
    t1 = int(idx[np.argmax(x[idx])])                # np.argmax: the first (lowest) index of the maximum
    ok[t1] = False
    idx = np.flatnonzero(ok)
    t2 = int(idx[np.argmax(x[idx])])
    return t1, t2


def margin_row(x, t1, t2):
    x = np.asarray(x, dtype=np.float32)
    return np.float32(x[t1] - x[t2])                # one fp32 subtraction


def logprob_row(x, pick, drop=None, twice=None):
    """log_softmax(x)[pick] in float64 on the fp32 values; NaN for a pick outside [0, n).  drop / twice: the self-check's mutations — entry
    `drop` left out of the sum, entry `twice` counted twice"""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    if not 0 <= pick < xd.shape[0]:
        return float("nan")
    m = xd.max()
    w = np.ones_like(xd)
    if drop is not None:
        w[drop] = 0.0
    if twice is not None:
        w[twice] = 2.0
    return float(xd[pick] - (m + np.log(np.sum(w * np.exp(xd - m)))))


def reference(logits, picks):
    """logits fp32 [B, n] (numpy or CPU tensor), picks [B] -> (logprob float64 [B], margin float32 [B], top2 int64 [B, 2])"""
    x = logits.numpy() if torch.is_tensor(logits) else np.asarray(logits, dtype=np.float32)
    B = x.shape[0]
    lp, mg, t2 = np.zeros(B), np.zeros(B, np.float32), np.zeros((B, 2), np.int64)
    for b in range(B):
        t2[b] = top2_row(x[b])
        mg[b] = margin_row(x[b], *t2[b])
        lp[b] = logprob_row(x[b], int(picks[b]))
    return lp, mg, t2


def pick_of_key(key):
    """the index in a packed (ordered value bits, ~index) key, as vg_decode_step_end decodes it"""
    return 0xFFFFFFFF - (int(key) & 0xFFFFFFFF)


# ------------------------------------------------------------------ the twin of the two ops functions, on CPU tensors
def token_scores_workspace(B, device):
    return torch.zeros(int(B), WS_INTS, dtype=torch.int32, device=device)


def token_scores_rows(logits, step, scores, top2, acc=None, tok=None, ws=None):
    assert logits.dim() == 2 and logits.dtype == torch.float32 and (acc is None) != (tok is None)
    B, n = logits.shape
    assert n >= 2 and 1 <= B <= 16 and scores.shape == top2.shape and scores.shape[-1] == 2
    cap = scores.numel() // (2 * B)
    sc, t2 = scores.view(B, cap, 2), top2.view(B, cap, 2)
    picks = [int(tok[b]) if tok is not None else pick_of_key(acc[b]) for b in range(B)]
    lp, mg, tt = reference(logits.detach().cpu().contiguous(), picks)
    for b in range(B):
        j = int(step[b])
        if 0 <= j < cap:
            sc[b, j, 0], sc[b, j, 1] = float(np.float32(lp[b])), float(mg[b])
            t2[b, j, 0], t2[b, j, 1] = int(tt[b, 0]), int(tt[b, 1])


# ------------------------------------------------------------------ crafted rows (self-check and GPU tests)
LOW = -28.0        # expf(LOW) * 2^40 < 1: the contract's fixed point sees no mass here (float64 sees < 1e-7 of the total over 2^17 entries)


def slice_bounds(n):
    """the kernel's slices of a row of n entries: up to 64 of at most 2048 entries (a function of n alone)"""
    nb = min(64, -(-n // 2048))
    chunk = -(-n // nb)
    return [(w * chunk, min(n, (w + 1) * chunk)) for w in range(nb)]


def crafted(kind, n=None):
    """(row fp32 [n], the indices that carry the mass).  "two": two entries (0 and -0.75) in a row at LOW; "slices": one entry per slice of the
    kernel, at another offset in each, values 0, -0.125, -0.25, ...; "flat": 2048 equal entries."""
    if kind == "flat":
        n = n or 2048
        return np.full(n, 1.25, np.float32), list(range(n))
    n = n or 32064
    x = np.full(n, LOW, np.float32)
    if kind == "two":
        at = [n // 3, n - 2]
        x[at[0]], x[at[1]] = 0.0, -0.75
        return x, at
    assert kind == "slices"
    at = []
    for w, (lo, hi) in enumerate(slice_bounds(n)):
        i = lo + (w * 131) % (hi - lo)
        x[i] = -0.125 * (w % 8)
        at.append(i)
    return x, at
