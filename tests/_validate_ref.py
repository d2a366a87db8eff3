"""The numpy statement of vg_logit_class_counts' contract (include/vg_kernels.h), written from the contract and not from the
reference: test infrastructure only, not collected.  `mutant` names one deliberate defect; tests/test_validate.py shows that the
fixture's crafted inputs tell every one of them from the statement.  logit_class_counts has the operator's signature, so that it
can stand in for it (monkeypatch) where the host-side code is exercised without a GPU."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validate.npz")
MUTANTS = ("ge", "nan_foreground", "ignore_kept_in_out", "ignore_counted_in_tgt", "stray_is_class_1")


def counts(logits, target, ignore_index=255, mutant=None):
    """logits [..., H, W] float array, target [..., H, W] integer array with values in 0..255 ->
    int64 [..., 6] = (inter0, inter1, out0, out1, tgt0, tgt1)"""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(logits, np.float32)
    t = np.asarray(target).astype(np.int64)
    assert x.shape == t.shape and x.ndim >= 2 and t.min(initial=0) >= 0 and t.max(initial=0) <= 255
    with np.errstate(invalid="ignore"):
        cls = (x >= 0) if mutant == "ge" else (x > 0)              # strictly positive; NaN compares false
    if mutant == "nan_foreground":
        cls = cls | np.isnan(x)
    if mutant == "stray_is_class_1":
        t = np.where((t > 1) & (t != ignore_index), 1, t)
    live = t != ignore_index                                       # an ignored pixel counts in nothing
    live_out = np.ones_like(live) if mutant == "ignore_kept_in_out" else live
    live_tgt = np.ones_like(live) if mutant == "ignore_counted_in_tgt" else live
    t_tgt = np.where(t == ignore_index, 1, t) if mutant == "ignore_counted_in_tgt" else t
    ax = (-2, -1)
    cols = []
    for k in (0, 1):
        cols.append((live & (t == k) & (cls == bool(k))).sum(ax))                 # inter[k]: target k and class k
    for k in (0, 1):
        cols.append((live_out & (cls == bool(k))).sum(ax))                        # out[k]: every live pixel, by class
    for k in (0, 1):
        cols.append((live_tgt & (t_tgt == k)).sum(ax))                            # tgt[k]: live pixels whose target is k
    return np.stack(cols, -1).astype(np.int64)


def triples(table):
    """int64 [..., 6] -> (area_intersection, area_union, area_target), int64 [..., 2] each: union = out + tgt - inter"""
    table = np.asarray(table)
    inter, out, tgt = table[..., 0:2], table[..., 2:4], table[..., 4:6]
    return inter, out + tgt - inter, tgt


def logit_class_counts(logits, target, ignore_index=255):
    """ops.logit_class_counts on host tensors"""
    return torch.from_numpy(counts(logits.detach().float().cpu().numpy(), target.detach().cpu().to(torch.int64).numpy(), ignore_index))


def fixture():
    return dict(np.load(FIXTURE))


def sample_frames(fx, s):
    """(logits float32 [T, H, W], target uint8 [T, H, W]) of sample s of the fixture's three samples"""
    return fx[f"s{s}_logits"], fx[f"s{s}_target"]
