"""Masks as COCO run-length codes without a GPU: the numpy statement (tests/_rle_ref.py) against the
reference's own mask_to_rle_pytorch / rle_to_mask / area_from_rle outputs (tests/golden/rle.npz, exact), the compressed string
codec, the host helpers of videoglamm_amd/postproc.py and the façade's return_rle / return_masks with ops.mask_rle /
ops.rle_to_mask replaced by the statement."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _golden as G
import _rle_ref as RR

torch.set_grad_enabled(False)


def gold():
    g = {k: v.numpy() for k, v in G.fixture("rle.npz").items()}
    W = int(g["shape"][2])
    g["masks"] = np.unpackbits(g["masks"], axis=-1, count=W).astype(bool)
    g["zero_masks"] = np.unpackbits(g["zero_masks"], axis=-1, count=W).astype(bool)
    return g


def codes(counts, offsets):
    return [counts[a:b].tolist() for a, b in zip(offsets[:-1], offsets[1:])]


# ------------------------------------------------------------------------------------------------ the statement == the reference
def test_statement_matches_reference():
    g = gold()
    n, H, W = g["shape"]
    assert g["masks"].shape == (n, H, W) == (33, 40, 50) and os.path.getsize(os.path.join(G.GOLD, "rle.npz")) < 64 * 1024
    counts, offsets = RR.codes_np(g["masks"])
    assert counts.dtype == np.int32 and offsets.dtype == np.int64
    assert np.array_equal(counts, g["counts"]) and np.array_equal(offsets, g["offsets"])
    ref = codes(g["counts"], g["offsets"])
    for c, m, a in zip(ref, g["masks"], g["area"]):
        assert RR.encode_np(m) == c and np.array_equal(RR.decode_np(c, H, W), m)
        assert sum(c[1::2]) == a == m.sum() and sum(c) == H * W
        assert len(c) == np.count_nonzero(np.diff(m.T.reshape(-1))) + 1 + int(m[0, 0])             # n_runs = len(P) + 1 + fg(0)
    assert ref[0] == [H * W] and ref[1] == [0, H * W]                                               # empty, full
    zero = codes(g["zero_counts"], g["zero_offsets"])
    assert any(0 in c[1:-1] for c in zero)
    for c, m in zip(zero, g["zero_masks"]):
        assert np.array_equal(RR.decode_np(c, H, W), m)
    assert RR.decode_np([H * W - 1], H, W) is None and RR.decode_np([H * W + 1], H, W) is None and RR.decode_np([-1, H * W + 1], H, W) is None
    # the rules at a column's end, spelled out
    H, W = 37, 53
    m = np.zeros((H, W), bool)
    m[H - 1, 20] = m[0, 21] = True
    assert RR.encode_np(m) == [21 * H - 1, 2, H * W - 21 * H - 1]                                   # one run of 2 across the column end
    m[0, 21], m[1, 21] = False, True
    assert RR.encode_np(m) == [21 * H - 1, 1, 1, 1, H * W - 21 * H - 2]
    m[:] = False
    m[0, 0] = m[H - 1, W - 1] = True
    assert RR.encode_np(m) == [0, 1, H * W - 2, 1]


# ------------------------------------------------------------------------------------------------ the compressed string
def test_string_codec():
    from videoglamm_amd import postproc as PP
    rle = {"size": [9, 10], "counts": [6, 1, 40, 4, 5, 4, 5, 4, 21]}
    enc = PP.coco_encode_rle(rle)
    assert enc == {"size": [9, 10], "counts": "61X13mN000`0"} and isinstance(enc["counts"], str)
    assert PP.coco_decode_rle(enc) == rle and PP.coco_decode_rle({"size": [9, 10], "counts": b"61X13mN000`0"}) == rle
    assert PP.coco_decode_rle(rle) == rle and PP.coco_encode_rle(enc) == enc                       # already in the form asked for
    assert PP.area_from_rle(rle) == PP.area_from_rle(enc) == 1 + 4 + 4 + 4
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        c = rng.choice([0, 0, 1, 2, 15, 16, 31, 32, 1023, 1024, 2 ** 15 - 1, 2 ** 15, 2 ** 15 + 1, 2 ** 20, 2 ** 30], size=n)
        c = (c + rng.integers(0, 3, size=n) * (c > 0)).tolist()
        s = PP.coco_encode_rle({"size": [1, 1], "counts": c})["counts"]
        assert all(48 <= ord(ch) < 48 + 64 for ch in s)
        assert PP.coco_decode_rle({"size": [1, 1], "counts": s})["counts"] == c, c
    big = {"size": [1024, 1024], "counts": [1024 * 1024]}
    s = PP.coco_encode_rle(big)
    assert PP.coco_decode_rle(s) == big and len(s["counts"]) == 5                                  # 2^20 plus its sign bit: 22 bits, five groups
    with pytest.raises(ValueError):
        PP.coco_decode_rle({"size": [1, 1], "counts": "a"})                                       # 'a' announces another group


# ------------------------------------------------------------------------------------------------ postproc on the statement
@pytest.fixture()
def host_rle(cpu_ops, monkeypatch):
    from videoglamm_amd import _lib, ops
    from videoglamm_amd import postproc as PP
    calls = []

    def mask_rle(masks):
        calls.append(tuple(masks.shape))
        return RR.mask_rle(masks)

    monkeypatch.setattr(ops, "mask_rle", mask_rle, raising=True)
    monkeypatch.setattr(ops, "rle_to_mask", RR.rle_to_mask, raising=True)
    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(PP, "DEVICE", "cpu")
    return calls


def test_postproc_matches_reference(host_rle):
    from videoglamm_amd import postproc as PP
    g = gold()
    n, H, W = (int(v) for v in g["shape"])
    ref = codes(g["counts"], g["offsets"])
    for m in (g["masks"], g["masks"].astype(np.uint8) * 255, torch.from_numpy(g["masks"]), g["masks"].astype(np.float32)):
        rles = PP.mask_to_rle_pytorch(m)
        assert [r["counts"] for r in rles] == ref and all(r["size"] == [H, W] and type(r["counts"][0]) is int for r in rles)
    assert PP.mask_to_rle_pytorch(np.zeros((0, 4, 5), bool)) == []
    assert [PP.area_from_rle(r) for r in rles] == g["area"].tolist()
    one = PP.rle_to_mask(rles[5])
    assert isinstance(one, np.ndarray) and one.dtype == bool and np.array_equal(one, g["masks"][5])
    packed = [PP.coco_encode_rle(r) for r in rles]
    for src in (rles, packed):
        back = PP.rle_to_mask(src)
        assert isinstance(back, list) and all(np.array_equal(b, m) for b, m in zip(back, g["masks"]))
    dev = PP.rle_to_mask(packed[7], device="cpu")
    assert torch.is_tensor(dev) and dev.dtype == torch.bool and np.array_equal(dev.numpy(), g["masks"][7])
    zero = [{"size": [H, W], "counts": c} for c in codes(g["zero_counts"], g["zero_offsets"])]
    assert all(np.array_equal(b, m) for b, m in zip(PP.rle_to_mask(zero), g["zero_masks"]))
    assert [PP.area_from_rle(r) for r in zero] == g["zero_area"].tolist()
    mixed = PP.rle_to_mask([rles[3], {"size": [2, 3], "counts": [1, 2, 3]}, rles[4]])            # sizes may differ inside a list
    assert np.array_equal(mixed[1], np.array([[0, 1, 0], [1, 0, 0]], bool)) and np.array_equal(mixed[2], g["masks"][4])
    for bad in ([H * W - 1], [H * W + 1], [5, -1, H * W - 4]):
        with pytest.raises(ValueError, match="code 1"):
            PP.rle_to_mask([rles[0], {"size": [H, W], "counts": bad}, rles[2]])


# ------------------------------------------------------------------------------------------------ the façade
def _build(**over):
    from test_oracle_e2e import e2e_setup
    from videoglamm_amd.model import VideoGLaMMForCausalLM
    fx, sd, cfg, inp = e2e_setup()
    kw = {k: over.pop(k) for k in ("min_blob_size",) if k in over}
    m = VideoGLaMMForCausalLM(sd, dict(cfg, **over), torch_dtype=torch.float32, device=torch.device("cpu"), **kw)
    args = ([inp["images"]], [inp["context_images"]], [inp["images_for_sam"]], inp["input_ids"][None], [(1024, 1024)], [inp["original_size"]])
    return m, args, inp


def check_codes(segs, rle, hw):
    """the codes have the masks' keys, and each decodes to its mask"""
    assert len(segs) == len(rle) == 1
    seg, code = segs[0], rle[0]
    assert len(seg) > 0 and list(seg) == list(code)
    for t in seg:
        assert list(seg[t]) == list(code[t])
        for k in seg[t]:
            c = code[t][k]
            assert c["size"] == list(hw) and isinstance(c["counts"], list) and all(type(v) is int for v in c["counts"])
            assert np.array_equal(RR.decode_np(c["counts"], *hw), seg[t][k] > 0), (t, k)


def test_facade_return_rle(host_rle, monkeypatch):
    m, args, inp = _build()
    hw = tuple(inp["original_size"])
    kw = dict(max_new_tokens=inp["max_new_tokens"], use_sam2_video_branch=False)
    ids, segs, rle = m.inference(*args, return_rle=True, **kw)
    calls = list(host_rle)
    ref = m.inference(*args, **kw)                                                # after the True call: the keyword does not stick
    assert isinstance(ref, tuple) and len(ref) == 2 and host_rle == calls         # the old tuple, and no encoding
    assert ids.equal(ref[0]) and isinstance(ref[1], list) and isinstance(ref[1][0], dict)
    seg, rseg = segs[0], ref[1][0]
    assert list(seg) == list(rseg) and all(np.array_equal(seg[t][k], rseg[t][k]) for t in rseg for k in rseg[t])
    check_codes(segs, rle, hw)
    T, N = len(seg), len(seg[0])
    assert calls == [(T, N) + hw]                                                 # ONE call over all T x N masks
    # without the dense download: the keys stay, the pixels are None, _to_host is never called
    spy = []
    monkeypatch.setattr(m, "_to_host", lambda x: spy.append(1) or x)
    ids2, segs2, rle2 = m.inference(*args, return_rle=True, return_masks=False, **kw)
    assert spy == [] and ids2.equal(ids)
    assert list(segs2[0]) == list(seg) and all(list(segs2[0][t]) == list(seg[t]) and all(v is None for v in segs2[0][t].values()) for t in seg)
    assert rle2 == rle


def test_facade_return_rle_with_boxes_after_the_blob_filter(host_rle, monkeypatch):
    """video branch, min_blob_size set, boxes fused with the filter: the boxes come first, the codes last, and the codes are those of the
    filtered masks that are returned"""
    import _boxes_ref as BR
    from videoglamm_amd import ops
    monkeypatch.setattr(ops, "mask_boxes", BR.mask_boxes, raising=True)
    m, args, inp = _build(min_blob_size=20)
    hw = tuple(inp["original_size"])
    out = m.inference(*args, return_boxes=True, return_rle=True, max_new_tokens=inp["max_new_tokens"], use_sam2_video_branch=True)
    assert len(out) == 4
    check_codes(out[1], out[3], hw)
    seg, box = out[1][0], out[2][0]
    assert list(box) == list(seg) and all(np.array_equal(box[t][k], BR.xyxy_np(seg[t][k])) for t in seg for k in seg[t])


def test_facade_refusals_and_no_seg(host_rle):
    m, args, inp = _build(seg_token_idx=10 ** 6)
    out = m.inference(*args, max_new_tokens=3, use_sam2_video_branch=True, return_rle=True)
    assert len(out) == 3 and out[1] == [{}] and out[2] == [{}] and host_rle == []
    out = m.inference(*args, max_new_tokens=3, use_sam2_video_branch=True, return_boxes=True, return_rle=True, return_masks=False)
    assert len(out) == 4 and out[1:] == ([{}], [{}], [{}])
    spy = []
    m._text_and_hiera = lambda *a, **k: spy.append(1)
    for fn in (m.inference, m.inference_framewise, m.inference_video_branch):
        with pytest.raises(ValueError, match="return_masks"):                     # before any work
            fn(*args, max_new_tokens=3, return_masks=False)
    with pytest.raises(ValueError, match="return_masks"):
        m.inference_prompts(*args[:3], [args[3][0]], *args[4:], max_new_tokens=3, return_masks=False)
    with pytest.raises(ValueError, match="return_masks"):
        m.inference_clips([args], max_new_tokens=3, return_masks=False)
    assert spy == []
    m.comm = object()                                                             # a multi-GPU model
    for kw in (dict(return_rle=True), dict(return_rle=True, return_masks=False), dict(return_boxes=True, return_masks=False)):
        with pytest.raises(NotImplementedError):
            m.inference(*args, max_new_tokens=3, **kw)
        with pytest.raises(NotImplementedError):
            m.inference_video_branch(*args, max_new_tokens=3, **kw)
    with pytest.raises(NotImplementedError, match="return_rle"):
        m.inference_framewise(*args, max_new_tokens=3, return_rle=True)
    assert spy == []


# ------------------------------------------------------------------------------------------------ ABI
def test_new_entry_points_are_declared_and_bound():
    from videoglamm_amd import _lib
    with open(os.path.join(os.path.dirname(G.HERE), "include", "vg_kernels.h")) as f:
        header = f.read()
    bound = inspect.getsource(_lib._sig)
    for name in ("vg_mask_rle_count", "vg_mask_rle_emit", "vg_rle_to_mask"):
        assert re.search(rf"\bint {name}\(", header) and f'"{name}"' in bound
    import __graft_entry__ as g
    g.build()
    _lib.load()
    assert {"vg_mask_rle_count", "vg_mask_rle_emit", "vg_rle_to_mask"} <= set(_lib.EXPORTS)
