"""The numpy statement of ops.mask_boxes (test infrastructure only): np.nonzero min / max / count per mask, after
oracle.postproc.remove_small_blobs when min_size is set.  Same signature as the operator, so that it can stand in for it
(monkeypatch) where the host-side code is exercised without a GPU."""
import numpy as np
import torch


def boxes_np(masks, min_size=0):
    """[..., H, W] array (nonzero = foreground) -> (int32 [..., 5] = (xmin, ymin, xmax, ymax, area), filtered bool masks)"""
    from oracle import postproc as op
    m = np.asarray(masks) != 0
    H, W = m.shape[-2:]
    flat = m.reshape(-1, H, W)
    if min_size > 0:
        flat = np.stack([op.remove_small_blobs(x, min_size) for x in flat]).astype(bool) if len(flat) else flat
    out = np.empty((len(flat), 5), np.int32)
    for n, x in enumerate(flat):
        ys, xs = np.nonzero(x)
        out[n] = (xs.min(), ys.min(), xs.max(), ys.max(), len(xs)) if len(xs) else (W, H, -1, -1, 0)
    return out.reshape(m.shape[:-2] + (5,)), flat.reshape(m.shape)


def xyxy_np(masks, min_size=0):
    """the float32 [..., 4] value masks_to_boxes gives: the table's first four numbers, [1e8, 1e8, 0, 0] for an empty mask"""
    t, _ = boxes_np(masks, min_size)
    out = t[..., :4].astype(np.float32)
    out[t[..., 4] == 0] = (1e8, 1e8, 0, 0)
    return out


def mask_boxes(masks, min_size=0, return_mask=False):
    m = masks.detach().cpu().numpy()
    t, kept = boxes_np(m, min_size)
    t = torch.from_numpy(t)
    if not return_mask:
        return t
    return t, (torch.from_numpy(kept.astype(np.uint8)) if min_size > 0 else (masks.view(torch.uint8) if masks.dtype == torch.bool else masks))
