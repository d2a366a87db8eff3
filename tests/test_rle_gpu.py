"""Masks as COCO run-length codes on the MI355X (vg_mask_rle_count / vg_mask_rle_emit / vg_rle_to_mask):
integer work, so every check is torch.equal against the numpy statement (tests/_rle_ref.py), which tests/test_rle.py pins to
the reference's own outputs (tests/golden/rle.npz); round trips; refusals; and end to end through return_rle."""
import numpy as np
import pytest
import torch

import _boxes_ref as BR
import _golden as G
import _rle_ref as RR

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(1, 1), (1, 17), (17, 1), (5, 7), (2, 15), (3, 16), (3, 17), (64, 64), (65, 63), (100, 130), (257, 1000)]
BATCHES = (1, 3, 8)
DENSITIES = (0.0, 1.0, 0.5, 0.001)


def random_masks(N, H, W, density, seed):
    """uint8 [N, H, W]: foreground bytes are 1, 2 or 255"""
    rng = np.random.default_rng(seed)
    fg = rng.random((N, H, W)) < density
    return (fg * rng.choice(np.array([1, 2, 255], np.uint8), size=(N, H, W))).astype(np.uint8)


def check(ops, cuda, m):
    """encode m (numpy, [..., H, W]) on the device: n_runs (through the offsets) and the counts equal the statement's; then the round trip"""
    dm = torch.from_numpy(m).to(cuda)
    counts, offsets = ops.mask_rle(dm)
    want_c, want_o = RR.codes_np(m)
    n = int(np.prod(m.shape[:-2]))
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int64 and counts.is_cuda and offsets.is_cuda
    assert tuple(offsets.shape) == (n + 1,) and torch.equal(offsets.cpu(), torch.from_numpy(want_o))
    assert torch.equal(counts.cpu(), torch.from_numpy(want_c))
    H, W = m.shape[-2:]
    back, status = ops.rle_to_mask(counts, offsets, H, W)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (n, H, W) and status.dtype == torch.int32
    assert not status.any() and torch.equal(back, (dm != 0).view(torch.uint8).reshape(n, H, W))
    return counts, offsets


# ------------------------------------------------------------------------------------------------ encode + round trip
@pytest.mark.parametrize("H,W", SHAPES)
def test_mask_rle_against_statement(cuda, H, W):
    from videoglamm_amd import ops
    for N in BATCHES:
        for d in DENSITIES:
            m = random_masks(N, H, W, d, seed=H * 1000 + W + N)
            counts, offsets = check(ops, cuda, m)
            cb, ob = ops.mask_rle(torch.from_numpy(m != 0).to(cuda))                                # bool input
            assert torch.equal(cb, counts) and torch.equal(ob, offsets)
    m = random_masks(6, H, W, 0.3, seed=9).reshape(2, 3, H, W)                                     # leading dimensions: 2 x 3 codes in order
    _, offsets = check(ops, cuda, m)
    assert offsets.numel() == 2 * 3 + 1


def test_constructed_masks(cuda):
    from videoglamm_amd import ops
    H, W = 37, 53
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((13, H, W), np.uint8)
    for n, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        m[n, y, x] = 1                      # a single pixel at each corner
    m[4, 11, :] = 2                         # one full row
    m[5, :, 29] = 255                       # one full column
    m[6, H - 1, 20] = m[6, 0, 21] = 1       # neighbours across a column end: one run of 2
    m[7, H - 1, 20] = m[7, 1, 21] = 1       # not neighbours: two runs
    m[8] = (yy + xx) % 2                    # checkerboard at odd H
    m[9] = (yy + xx + 1) % 2
    m[10, 5:9, 6:40] = 1                    # masks 10 and 12 with the empty mask 11 between them: no state leaks
    m[12, 20:30, 1:3] = 1
    counts, offsets = check(ops, cuda, m)
    code = lambda n: counts[offsets[n]:offsets[n + 1]].tolist()
    assert code(0) == [0, 1, H * W - 1] and code(3) == [H * W - 1, 1]                              # the leading 0; a code that ends on foreground
    assert code(1) == [(W - 1) * H, 1, H - 1] and code(2) == [H - 1, 1, (W - 1) * H]
    assert len(code(4)) == 2 * W + 1 and code(5) == [29 * H, H, (W - 29 - 1) * H]
    assert code(6) == [21 * H - 1, 2, H * W - 21 * H - 1]
    assert code(7) == [21 * H - 1, 1, 1, 1, H * W - 21 * H - 2]
    assert code(8) == [1] * (H * W) and code(9) == [0] + [1] * (H * W)                             # odd H: the colour alternates across column ends too
    assert code(11) == [H * W]
    m[4, :11] = m[4, 12:] = 0
    m[4, 11, :] = 0
    m[4, 0, :] = 1                          # the first row: pixel 0 is foreground, 2W + 1 counts with the leading 0
    assert len(RR.encode_np(m[4])) == 2 * W + 1
    check(ops, cuda, m[4:5])
    H = 36                                  # even H: a column's last pixel equals the next column's first, the runs merge
    yy, xx = np.mgrid[:H, :W]
    e = np.stack([(yy + xx) % 2, (yy + xx + 1) % 2]).astype(np.uint8)
    counts, offsets = check(ops, cuda, e)
    assert counts[:offsets[1]].tolist() == [1] * (H - 1) + ([2] + [1] * (H - 2)) * (W - 1) + [1]
    for W in (15, 17, 31, 33, 63, 65):      # foreground in the last column group only
        for k in range(1, 5):
            m = np.zeros((2, 9, W), np.uint8)
            m[1, 2:7, W - k] = 3
            m[1, 8, W - 1] = 1
            check(ops, cuda, m)


@pytest.fixture(scope="module")
def full_size():
    from oracle import postproc as OP
    m = np.zeros((4, 1024, 1024), np.uint8)
    m[0] = OP.blobs((1024, 1024), 3, density=0.3) * 255
    m[2, 1023, 1023] = 1
    m[3] = random_masks(1, 1024, 1024, 0.5, seed=1)[0]
    return m, RR.codes_np(m)


def test_full_size(cuda, full_size):
    from videoglamm_amd import ops
    m, (want_c, want_o) = full_size
    dm = torch.from_numpy(m).to(cuda)
    counts, offsets = ops.mask_rle(dm)
    assert torch.equal(offsets.cpu().diff(), torch.from_numpy(want_o).diff())                      # n_runs first
    assert torch.equal(counts.cpu(), torch.from_numpy(want_c))
    back, status = ops.rle_to_mask(counts, offsets, 1024, 1024)
    assert not status.any() and torch.equal(back, (dm != 0).view(torch.uint8))


def test_unaligned_views(cuda):
    """a mask whose base is aligned to nothing (a view at a byte offset), at a W that is no multiple of the lane group"""
    from videoglamm_amd import ops
    for (H, W), N in (((5, 7), 3), ((65, 63), 2), ((33, 130), 2)):
        m = random_masks(N, H, W, 0.3, seed=N + H)
        want_c, want_o = RR.codes_np(m)
        for off in (1, 2, 3):
            base = torch.zeros(N * H * W + off, dtype=torch.uint8, device=cuda)
            view = base[off:].view(N, H, W)
            view.copy_(torch.from_numpy(m))
            counts, offsets = ops.mask_rle(view)
            assert torch.equal(counts.cpu(), torch.from_numpy(want_c)) and torch.equal(offsets.cpu(), torch.from_numpy(want_o))


# ------------------------------------------------------------------------------------------------ decode alone
def test_decode_fixture_codes(cuda):
    from videoglamm_amd import ops
    from videoglamm_amd import postproc as PP
    g = {k: v.numpy() for k, v in G.fixture("rle.npz").items()}
    n, H, W = (int(v) for v in g["shape"])
    for key in ("", "zero_"):
        want = np.unpackbits(g[key + "masks"], axis=-1, count=W)
        out, status = ops.rle_to_mask(torch.from_numpy(g[key + "counts"]).to(cuda), torch.from_numpy(g[key + "offsets"]).to(cuda), H, W)
        assert not status.any() and torch.equal(out.cpu(), torch.from_numpy(want))
    masks = np.unpackbits(g["masks"], axis=-1, count=W).astype(bool)
    rles = PP.mask_to_rle_pytorch(masks)                                                          # the reference's names, host lists in and out
    assert [v for r in rles for v in r["counts"]] == g["counts"].tolist() and [PP.area_from_rle(r) for r in rles] == g["area"].tolist()
    back = PP.rle_to_mask([PP.coco_encode_rle(r) for r in rles], device=cuda)
    assert all(b.is_cuda and b.dtype == torch.bool for b in back) and torch.equal(torch.stack(back).cpu(), torch.from_numpy(masks))
    assert np.array_equal(PP.rle_to_mask(rles[12]), masks[12])


@pytest.mark.parametrize("H,W", [(5, 7), (37, 53), (64, 64)])
def test_refusals(cuda, H, W):
    """a code that cannot be a mask of this size is refused: status 1, its mask all zero, its neighbours exact, nothing outside `out` touched"""
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    m = random_masks(2, H, W, 0.4, seed=H)
    a, b = RR.encode_np(m[0]), RR.encode_np(m[1])
    L = H * W
    for bad in ([3, L - 4], [3, L - 2], [L + 1], [L - 1], [5, -1, L - 4], [-L, 2 * L], [L, -1, 1], [2 ** 31 - 1, 2 ** 31 - 1, 2], []):
        assert sum(bad) != L or min(bad) < 0
        counts = torch.tensor(a + bad + b, dtype=torch.int32, device=cuda)
        offsets = torch.tensor([0, len(a), len(a) + len(bad), len(a) + len(bad) + len(b)], dtype=torch.int64, device=cuda)
        buf = torch.full((3 * L + 4096,), 0xAB, dtype=torch.uint8, device=cuda)                   # `out`, then a guard region
        status = torch.full((3,), 7, dtype=torch.int32, device=cuda)
        ends = torch.empty_like(counts)
        rc = lib.vg_rle_to_mask(ops._p(counts), ops._p(offsets), ops._p(buf), ops._p(status), ops._p(ends), 3, H, W, ops._stream())
        assert rc == 0
        out = buf[:3 * L].view(3, H, W).cpu()
        assert status.tolist() == [0, 1, 0], bad
        assert not out[1].any() and torch.equal(out[0], torch.from_numpy(m[0] != 0).to(torch.uint8)) and torch.equal(out[2], torch.from_numpy(m[1] != 0).to(torch.uint8))
        assert bool((buf[3 * L:] == 0xAB).all())
        o2, s2 = ops.rle_to_mask(counts, offsets, H, W)
        assert s2.tolist() == [0, 1, 0] and torch.equal(o2.cpu(), out)
    with pytest.raises(ValueError):
        ops.rle_to_mask(counts, torch.tensor([0, 5, 3, counts.numel()], dtype=torch.int64, device=cuda), H, W)       # offsets that decrease
    with pytest.raises(ValueError):
        ops.rle_to_mask(counts, torch.tensor([0, counts.numel() + 1], dtype=torch.int64, device=cuda), H, W)        # ... or run past the counts


def test_chained_calls_share_a_workspace(cuda):
    """two encodes on one stream through ONE workspace tensor, different masks: the second must not see the first one's scans"""
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    N, H, W = 3, 65, 63
    U = lib.vg_mask_rle_units(H, W)
    assert U == W * 2                                                                            # two segments of 64 rows at H = 65
    ws = torch.full((N, 4, U), -12345, dtype=torch.int32, device=cuda)
    res = []
    for seed, d in ((1, 0.5), (2, 0.01), (3, 0.9)):
        m = random_masks(N, H, W, d, seed=seed)
        m[seed % N] = 0
        dm = torch.from_numpy(m).to(cuda)
        n_runs = torch.empty(N, dtype=torch.int32, device=cuda)
        assert lib.vg_mask_rle_count(ops._p(dm), ops._p(ws), ops._p(n_runs), N, H, W, ops._stream()) == 0
        offsets = torch.zeros(N + 1, dtype=torch.int64, device=cuda)
        offsets[1:] = n_runs.cumsum(0)
        counts = torch.full((int(offsets[-1]) + 64,), -7, dtype=torch.int32, device=cuda)           # 64 sentinels behind the code
        assert lib.vg_mask_rle_emit(ops._p(dm), ops._p(ws), ops._p(offsets), ops._p(counts), N, H, W, ops._stream()) == 0
        res.append((m, dm, counts, offsets))                                                     # no synchronisation between the calls
    for m, dm, counts, offsets in res:
        want_c, want_o = RR.codes_np(m)
        assert torch.equal(offsets.cpu(), torch.from_numpy(want_o))
        assert torch.equal(counts[:-64].cpu(), torch.from_numpy(want_c)) and bool((counts[-64:] == -7).all())


def test_argument_errors(cuda):
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    N, H, W = 2, 8, 9
    m = torch.ones((N, H, W), dtype=torch.uint8, device=cuda)
    ws = torch.empty((N, 4, lib.vg_mask_rle_units(H, W)), dtype=torch.int32, device=cuda)
    assert lib.vg_mask_rle_units(H, W) == W and lib.vg_mask_rle_units(0, W) == 0 and lib.vg_mask_rle_units(1 << 16, 1 << 15) == 0 and lib.vg_mask_rle_units(2, 1 << 29) == 0 \
        and lib.vg_mask_rle_units(2, (1 << 29) - 1) == (1 << 29) - 1
    runs = torch.full((N,), 77, dtype=torch.int32, device=cuda)
    offs = torch.tensor([0, 2, 4], dtype=torch.int64, device=cuda)
    cnt = torch.full((4,), 77, dtype=torch.int32, device=cuda)
    out = torch.full((N, H, W), 77, dtype=torch.uint8, device=cuda)
    st = ops._stream()
    p = ops._p
    bad = [("vg_mask_rle_count", (None, p(ws), p(runs), N, H, W)), ("vg_mask_rle_count", (p(m), None, p(runs), N, H, W)),
           ("vg_mask_rle_count", (p(m), p(ws), None, N, H, W)), ("vg_mask_rle_count", (p(m), p(ws), p(runs), 0, H, W)),
           ("vg_mask_rle_count", (p(m), p(ws), p(runs), 65536, H, W)), ("vg_mask_rle_count", (p(m), p(ws), p(runs), N, 1 << 16, 1 << 15)),
           ("vg_mask_rle_count", (p(m), p(ws), p(runs), N, 2, 1 << 29)),                          # 4 planes of 2^29 units: past int indexing
           ("vg_mask_rle_emit", (p(m), p(ws), None, p(cnt), N, H, W)), ("vg_mask_rle_emit", (p(m), p(ws), p(offs), None, N, H, W)),
           ("vg_mask_rle_emit", (p(m), p(ws), p(offs), p(cnt), N, 0, W)),
           ("vg_rle_to_mask", (p(cnt), None, p(out), p(runs), p(cnt), N, H, W)), ("vg_rle_to_mask", (p(cnt), p(offs), None, p(runs), p(cnt), N, H, W)),
           ("vg_rle_to_mask", (p(cnt), p(offs), p(out), None, p(cnt), N, H, W)), ("vg_rle_to_mask", (p(cnt), p(offs), p(out), p(runs), None, N, H, W)),
           ("vg_rle_to_mask", (p(cnt), p(offs), p(out), p(runs), p(cnt), N, H, 0))]
    for fn, args in bad:
        assert getattr(lib, fn)(*args, st) != 0, (fn, args)
        assert fn.encode() in lib.vg_last_error()
    torch.cuda.synchronize()
    assert bool((runs == 77).all()) and bool((cnt == 77).all()) and bool((out == 77).all())         # nothing was launched
    counts, offsets = ops.mask_rle(torch.zeros((0, 4, 4), dtype=torch.uint8, device=cuda))         # no masks: no codes
    assert counts.numel() == 0 and offsets.tolist() == [0]
    o, s = ops.rle_to_mask(counts, offsets, 4, 4)
    assert tuple(o.shape) == (0, 4, 4) and s.numel() == 0
    o, s = ops.rle_to_mask(counts, torch.zeros(3, dtype=torch.int64, device=cuda), 4, 4)           # two empty codes: refused, nothing read
    assert s.tolist() == [1, 1] and not o.any()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def micro(cuda):
    import test_clips_gpu as TC
    return TC._micro(cuda)


def check_twin(ref, got, hw):
    """got = (ids, [segments], [codes]) of a return_rle call, ref = the plain call's pair: same ids, same masks, and the codes decode to them"""
    assert len(ref) == 2 and len(got) == 3 and torch.equal(got[0], ref[0])
    assert len(got[1]) == len(got[2]) == len(ref[1]) == 1
    seg, rseg, code = got[1][0], ref[1][0], got[2][0]
    assert list(seg) == list(rseg) == list(code)
    for t in seg:
        assert list(seg[t]) == list(rseg[t]) == list(code[t])
        for k in seg[t]:
            assert np.array_equal(seg[t][k], rseg[t][k])
            c = code[t][k]
            assert c["size"] == list(hw) and c["counts"] == RR.encode_np(seg[t][k]), (t, k)
            assert np.array_equal(RR.decode_np(c["counts"], *hw), seg[t][k])
    return len(seg)


@pytest.mark.parametrize("blob", [0, 20])
@pytest.mark.parametrize("video", [False, True])
def test_inference_return_rle(micro, video, blob, monkeypatch):
    m, clips = micro
    monkeypatch.setattr(m, "min_blob_size", blob)
    hw = clips[0][5][0]
    kw = dict(max_new_tokens=8, use_sam2_video_branch=video)
    ref = m.inference(*clips[0], **kw)
    got = m.inference(*clips[0], return_rle=True, **kw)
    assert check_twin(ref, got, hw) == 3
    assert len(m.inference(*clips[0], **kw)) == 2
    boxes = m.inference(*clips[0], return_boxes=True, **kw)
    both = m.inference(*clips[0], return_boxes=True, return_rle=True, **kw)
    assert len(both) == 4 and both[3] == got[2] and list(both[2][0]) == list(boxes[2][0])
    assert all(np.array_equal(both[2][0][t][k], boxes[2][0][t][k]) and np.array_equal(both[2][0][t][k], BR.xyxy_np(ref[1][0][t][k]))
               for t in boxes[2][0] for k in boxes[2][0][t])
    spy = []
    to_host = m._to_host
    monkeypatch.setattr(m, "_to_host", lambda x: spy.append(1) or to_host(x))
    lean = m.inference(*clips[0], return_rle=True, return_masks=False, **kw)                      # no dense download
    assert spy == [] and torch.equal(lean[0], ref[0]) and lean[2] == got[2]
    assert list(lean[1][0]) == list(ref[1][0]) and all(list(lean[1][0][t]) == list(ref[1][0][t]) and set(lean[1][0][t].values()) == {None} for t in ref[1][0])
    with pytest.raises(ValueError, match="return_masks"):
        m.inference(*clips[0], return_masks=False, **kw)


@pytest.mark.parametrize("video", [False, True])
def test_clips_and_prompts_return_rle(micro, video, monkeypatch):
    m, clips = micro
    monkeypatch.setattr(m, "min_blob_size", 20 if video else 0)
    kw = dict(max_new_tokens=8, use_sam2_video_branch=video)
    single = [m.inference(*c, return_rle=True, **kw) for c in clips[:2]]
    ref = m.inference_clips(clips[:2], **kw)
    got = m.inference_clips(clips[:2], return_rle=True, **kw)
    assert len(ref) == len(got) == 2
    for r, g, s, c in zip(ref, got, single, clips):
        check_twin(r, g, c[5][0])
        assert g[2] == s[2]                                                                      # the codes of the single call
    images, context, sam, ids, resize, hw = clips[0]
    n0 = int((ids[0] == -200).nonzero().max()) + 1
    prompts = [ids[0], torch.cat([ids[0][:n0], torch.tensor([84, 12, 99, 150, 7])])]
    for shared in (True, False):
        ref = m.inference_prompts(images, context, sam, prompts, resize, hw, shared=shared, **kw)
        got = m.inference_prompts(images, context, sam, prompts, resize, hw, shared=shared, return_rle=True, **kw)
        assert len(ref) == 2 and len(got) == 3 and len(got[0]) == len(got[1]) == len(got[2]) == 2
        for b in range(2):
            check_twin((ref[0][b], [ref[1][b]]), (got[0][b], [got[1][b]], [got[2][b]]), hw[0])
        if not shared:                                                                           # one inference() per prompt: its codes
            for b in range(2):
                alone = m.inference(images, context, sam, prompts[b][None], resize, hw, return_rle=True, **kw)
                assert got[2][b] == alone[2][0]
    lean = m.inference_prompts(images, context, sam, prompts, resize, hw, shared=True, return_rle=True, return_boxes=True, return_masks=False, **kw)
    assert len(lean) == 4 and all(v is None for s in lean[1] for fr in s.values() for v in fr.values())
