"""The numpy statement of ops.mask_rle / ops.rle_to_mask (test infrastructure only): COCO's uncompressed run-length code in
mask_to_rle_pytorch's form.  mask_rle / rle_to_mask have the operators' signatures, so that they can stand in for them
(monkeypatch) where the host-side code is exercised without a GPU."""
import numpy as np
import torch


def encode_np(mask):
    """[H, W] array (nonzero = foreground) -> list of counts: runs of the column-major pixel order, a leading 0 when pixel 0 is foreground"""
    f = (np.asarray(mask) != 0).T.reshape(-1)
    p = np.flatnonzero(f[1:] != f[:-1]) + 1
    return ([0] if f[0] else []) + np.diff(np.concatenate(([0], p, [f.size]))).tolist()


def decode_np(counts, h, w):
    """counts -> bool [h, w]; None when a count is negative or they do not sum to h * w.  Pixel j lies in the first run that ends beyond j."""
    c = np.asarray(counts, np.int64).reshape(-1)
    if (c < 0).any() or c.sum() != h * w:
        return None
    idx = np.searchsorted(np.cumsum(c), np.arange(h * w), side="right")
    return (idx & 1).astype(bool).reshape(w, h).T


def codes_np(masks):
    """[..., H, W] -> (counts int32 [total], offsets int64 [n + 1]) of the flattened leading dimensions"""
    m = np.asarray(masks)
    flat = m.reshape((-1,) + m.shape[-2:])
    codes = [encode_np(x) for x in flat]
    offsets = np.concatenate(([0], np.cumsum([len(c) for c in codes], dtype=np.int64))).astype(np.int64)
    return np.array([v for c in codes for v in c], np.int32), offsets


def mask_rle(masks):
    counts, offsets = codes_np(masks.detach().cpu().numpy())
    return torch.from_numpy(counts), torch.from_numpy(offsets)


def rle_to_mask(counts, offsets, H, W):
    c, o = counts.detach().cpu().numpy(), offsets.detach().cpu().numpy()
    n = len(o) - 1
    out, status = np.zeros((n, H, W), np.uint8), np.zeros(n, np.int32)
    for i in range(n):
        m = decode_np(c[o[i]:o[i + 1]], H, W)
        if m is None:
            status[i] = 1
        else:
            out[i] = m
    return torch.from_numpy(out), torch.from_numpy(status)
