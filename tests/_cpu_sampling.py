"""CPU statement of the sampled decoding contract: HF's Temperature -> TopK -> TopP warpers as transformers 4.41
writes them, the kept set and its inverse CDF in float64, and a numpy Philox4x32-10."""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: uint32 [..., 2] (numpy) -> uint32 [..., 4] (Random123's philox4x32 with 10 rounds)."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[..., 0], dtype=np.uint64), np.asarray(key[..., 1], dtype=np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    for r in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_x0(seed, step):
    """word 0 of philox4x32_10(key = seed (64 bit), counter = (step, 0, 0, 0)) for arrays of seeds / steps"""
    seed = np.asarray(seed, dtype=np.uint64)
    step = np.asarray(step, dtype=np.uint64)
    ctr = np.stack([step, 0 * step, 0 * step, 0 * step], axis=-1)
    key = np.stack([seed & np.uint64(0xFFFFFFFF), seed >> np.uint64(32)], axis=-1)
    return philox4x32_10(ctr, key)[..., 0]


def uniform(seed, step):
    return float(int(philox_x0(seed, step)) >> 8) * 2.0 ** -24


def hf_warp(scores, T, k, p):
    """transformers 4.41 TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper (min_tokens_to_keep = 1) on a float32 torch row [1, V]"""
    scores = scores.clone()
    if T != 1.0:
        scores = scores / T
    if k != 0:
        kk = min(max(k, 1), scores.size(-1))
        remove = scores < torch.topk(scores, kk)[0][..., -1, None]
        scores = scores.masked_fill(remove, -float("inf"))
    if p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cum = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        sorted_remove = cum <= (1 - p)
        sorted_remove[..., -1:] = 0
        remove = sorted_remove.scatter(1, sorted_indices, sorted_remove)
        scores = scores.masked_fill(remove, -float("inf"))
    return scores


def kept(x, T, k, p):
    """the contract in float64: -> (indices in draw order (descending y, ties ascending index), probabilities, margin of the top-p cut to 1 - p)"""
    x = np.asarray(x, dtype=np.float32)
    y = (x / np.float32(T)).astype(np.float32) if T != 1.0 else x.copy()
    n = y.size
    order = np.lexsort((np.arange(n), -y.astype(np.float64)))          # descending y, ties by ascending index
    ys = y[order].astype(np.float64)
    if k != 0 and k < n:
        thr = ys[k - 1]
        m = int(np.sum(ys >= thr))
        order, ys = order[:m], ys[:m]
    e = np.exp(ys - ys[0])
    prob = e / e.sum()
    margin = np.inf
    if p < 1.0:
        above = np.concatenate([[0.0], np.cumsum(prob)[:-1]])          # mass strictly above each entry
        asc_cum = 1.0 - above                                          # its ascending cumulative probability
        keep = asc_cum > 1.0 - p
        keep[0] = True
        margin = float(np.min(np.abs(asc_cum - (1.0 - p))))
        order, ys = order[keep], ys[keep]
        e = np.exp(ys - ys[0])
        prob = e / e.sum()
    return order, prob, margin


def draw(order, prob, u):
    """inverse CDF in the given order -> (index, distance of u to the nearest CDF edge)"""
    cdf = np.cumsum(prob)
    j = int(np.searchsorted(cdf, u, side="right"))
    j = min(j, len(order) - 1)
    edge = float(np.min(np.abs(np.concatenate([[0.0], cdf]) - u)))
    return int(order[j]), edge
