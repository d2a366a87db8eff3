"""Golden vectors of the validation metrics gIoU / cIoU (tests/golden/validate.npz).

Runs in the build container only: it executes the reference's OWN intersectionAndUnionGPU and AverageMeter (utils/utils.py)
and the validator's own statements (utils/trainer.py:442-456 per sample, :463-465 at the end), compiled from the files where
they lie, on small inputs made here, on the CPU, and records inputs and outputs.  Nothing of the reference is copied; tests read
the .npz only.  The label tensors go in as float32 (CPU histc refuses integers), which leaves their values unchanged.

  python tests/golden/make_golden_validate.py
"""
import ast
import os
import sys
import textwrap
from enum import Enum

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as ri  # noqa: E402

H, W, IGNORE = 37, 53, 255
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45], np.float32)      # 1e-45 is the smallest positive denormal


def classes(relpath, names, namespace):
    """_ref_import.functions for top-level classes"""
    path = os.path.join(ri.R, relpath)
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    picked = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    assert {n.name for n in picked} == set(names), names
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), namespace)
    return [namespace[n] for n in names]


def statements(relpath, first, last, must_hold):
    """lines first..last (1-based, inclusive) of a reference file as a code object; must_hold: text those lines have to contain,
    so that a reference whose lines moved is noticed"""
    path = os.path.join(ri.R, relpath)
    with open(path) as f:
        src = "".join(f.readlines()[first - 1:last])
    assert all(s in src for s in must_hold), (relpath, first, last)
    return compile("\n" * (first - 1) + textwrap.dedent(src), path, "exec")


def blob(rng, T):
    """targets uint8 [T, H, W]: an ellipse that drifts, 0 / 1"""
    yy, xx = np.mgrid[:H, :W]
    cy, cx = rng.uniform(10, H - 10), rng.uniform(12, W - 12)
    out = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        out[t] = ((yy - cy - t) / 7.0) ** 2 + ((xx - cx + 2 * t) / 11.0) ** 2 <= 1
    return out


def make_samples():
    """three samples of T = 3, 4, 5 frames.  Logits: half-integers in [-2, 2] (many exact zeros), close to the target so that the
    IoUs are not trivial, with the special values planted on target 0, target 1 and ignored pixels."""
    rng = np.random.default_rng(20260)
    samples = []
    for s, T in enumerate((3, 4, 5)):
        tgt = blob(rng, T)
        x = (rng.integers(-4, 5, size=(T, H, W)) * 0.5).astype(np.float32)
        x = np.where(rng.random((T, H, W)) < 0.7, np.where(tgt == 1, np.abs(x) + 0.5, -np.abs(x)), x).astype(np.float32)
        tgt[:, :, W - 4:] = IGNORE                                   # an ignore band over every frame, crossing nothing or the blob
        tgt[:, 5:8, 20:30] = IGNORE
        for t in range(T):                                           # the special values on a target-0 row, a target-1 row, the band
            ys, xs = np.nonzero(tgt[t] == 1)
            for k, v in enumerate(SPECIAL):
                x[t, 0, 2 + k] = v
                x[t, 6, 21 + k] = v
                if len(ys) > k:
                    x[t, ys[k], xs[k]] = v
        if s == 0:
            tgt[1] = 0                                               # frame 1: no object in the target, none predicted: union[1] == 0
            x[1] = -np.abs(x[1])
            tgt[2] = IGNORE                                          # frame 2: entirely ignore label: both unions are 0
        if s == 1:
            tgt[0, 30:33, 3:40] = 7                                  # a stray label: counted by the prediction's histogram only
            x[0, 30:33, 3:40:2] = 1.5
        samples.append((x, tgt))
    return samples


def main():
    ns = {"torch": torch, "np": np, "Enum": Enum}
    (intersectionAndUnionGPU,) = ri.functions("utils/utils.py", ["intersectionAndUnionGPU"], ns)
    Summary, AverageMeter = classes("utils/utils.py", ["Summary", "AverageMeter"], ns)
    per_sample = statements("utils/trainer.py", 442, 456, ["intersectionAndUnionGPU(", "acc_iou[union_i == 0] += 1.0", "acc_iou_meter.update("])
    final = statements("utils/trainer.py", 463, 465, ["iou_class = ", "ciou = ", "giou = "])

    def triple(x, tgt):
        i, u, t = intersectionAndUnionGPU(torch.from_numpy((x > 0).astype(np.float32)).clone(), torch.from_numpy(tgt.astype(np.float32)),
                                          2, ignore_index=IGNORE)
        assert max(float(v.max()) for v in (i, u, t)) < 2 ** 24      # the float32 histograms are exact
        return np.stack([v.numpy().astype(np.int64) for v in (i, u, t)])

    out = {"ignore_index": np.array(IGNORE, np.int64)}
    env = dict(ns, intersectionAndUnionGPU=intersectionAndUnionGPU,
               intersection_meter=AverageMeter("Intersec", ":6.3f", Summary.SUM), union_meter=AverageMeter("Union", ":6.3f", Summary.SUM),
               acc_iou_meter=AverageMeter("gIoU", ":6.3f", Summary.SUM))
    for s, (x, tgt) in enumerate(make_samples()):
        with np.errstate(invalid="ignore"):
            out[f"s{s}_logits"], out[f"s{s}_target"] = x, tgt
            out[f"s{s}_triples"] = np.stack([triple(a, b) for a, b in zip(x, tgt)])            # [T, 3, 2]
            env["masks_list"] = torch.from_numpy(tgt.astype(np.float32))                       # [T, H, W], as trainer.py:416 leaves it
            env["output_list"] = torch.from_numpy((x > 0).astype(np.float32))                  # trainer.py:421-423
        exec(per_sample, env)
        out[f"s{s}_intersection"], out[f"s{s}_union"], out[f"s{s}_acc_iou"] = env["intersection"], env["union"], env["acc_iou"]
        out[f"s{s}_n"] = np.array(tgt.shape[0], np.int64)
    exec(final, env)
    out["giou"], out["ciou"] = np.asarray(env["giou"]), np.asarray(env["ciou"])
    # one 1 x 1 frame per (special value, target label): the smallest mask there is
    ox = np.repeat(np.concatenate([SPECIAL, np.array([1.0, -1.0], np.float32)]), 4).reshape(-1, 1, 1)
    ot = np.tile(np.array([0, 1, IGNORE, 7], np.uint8), len(ox) // 4).reshape(-1, 1, 1)
    with np.errstate(invalid="ignore"):
        out["one_logits"], out["one_target"] = ox, ot
        out["one_triples"] = np.stack([triple(a, b) for a, b in zip(ox, ot)])
    path = os.path.join(HERE, "validate.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, f"{os.path.getsize(path) / 1e3:.1f} kB")
    print("giou", out["giou"], "ciou", out["ciou"])


if __name__ == "__main__":
    main()
