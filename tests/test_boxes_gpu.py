"""Boxes from masks on the MI355X (vg_mask_boxes / vg_blob_boxes): integer reductions, so every check is
torch.equal — against the numpy statement (tests/_boxes_ref.py), against the two-call chain remove_small_blobs -> mask_boxes,
against the reference's own masks_to_boxes outputs (tests/golden/grounding.npz), and end to end through return_boxes."""
import ctypes

import numpy as np
import pytest
import torch

import _boxes_ref as BR
import _golden as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(1, 1), (1, 17), (5, 7), (2, 15), (3, 16), (3, 17), (64, 64), (65, 63), (100, 130), (257, 1000)]
BATCHES = (1, 3, 8)
DENSITIES = (0.0, 1.0, 0.5, 0.001)


def random_masks(N, H, W, density, seed):
    """uint8 [N, H, W]: foreground bytes are 1, 2 or 255"""
    rng = np.random.default_rng(seed)
    fg = rng.random((N, H, W)) < density
    return (fg * rng.choice(np.array([1, 2, 255], np.uint8), size=(N, H, W))).astype(np.uint8)


def table(m):
    return torch.from_numpy(BR.boxes_np(m)[0])


def check(ops, cuda, m):
    got = ops.mask_boxes(torch.from_numpy(m).to(cuda))
    assert got.dtype == torch.int32 and tuple(got.shape) == m.shape[:-2] + (5,)
    assert torch.equal(got.cpu(), table(m))
    return got


# ------------------------------------------------------------------------------------------------ mask_boxes
@pytest.mark.parametrize("H,W", SHAPES)
def test_mask_boxes_against_statement(cuda, H, W):
    from videoglamm_amd import ops
    for N in BATCHES:
        for d in DENSITIES:
            m = random_masks(N, H, W, d, seed=H * 1000 + W + N)
            got = check(ops, cuda, m)
            assert torch.equal(ops.mask_boxes(torch.from_numpy(m != 0).to(cuda)), got)         # bool input
    m = random_masks(6, H, W, 0.3, seed=9).reshape(2, 3, H, W)                                # leading dimensions are kept
    check(ops, cuda, m)


def test_mask_boxes_full_size(cuda):
    from videoglamm_amd import ops
    m = random_masks(8, 1024, 1024, 0.5, seed=1)
    m[1] = 0
    m[2] = random_masks(1, 1024, 1024, 1e-6 * 3, seed=2)[0]       # a handful of pixels
    m[3, :, :] = 0
    m[3, 1023, 1023] = 7
    m[4, 100:900, 17:1001] = (m[4, 100:900, 17:1001] != 0) * 255
    m[4, :100] = 0
    m[4, 900:] = 0
    m[4, :, :17] = 0
    m[4, :, 1001:] = 0
    check(ops, cuda, m)


def test_constructed_masks(cuda):
    from videoglamm_amd import ops
    H, W = 37, 53
    m = np.zeros((9, H, W), np.uint8)
    for n, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        m[n, y, x] = 1                      # a single pixel at each corner
    m[4, 11, :] = 2                         # one full row
    m[5, :, 29] = 255                       # one full column
    m[6, 5:9, 6:40] = 1                     # masks 6 and 8 with the empty mask 7 between them: no state leaks
    m[8, 20:30, 1:3] = 1
    got = check(ops, cuda, m)
    assert got[7].tolist() == [W, H, -1, -1, 0] and got[3].tolist() == [W - 1, H - 1, W - 1, H - 1, 1]
    for W in (15, 17, 31, 33):              # only (y, W-1) and (y+1, 0): a 16-byte word straddles the row end
        for y in range(0, 6):
            m = np.zeros((2, 8, W), np.uint8)
            m[1, y, W - 1] = m[1, y + 1, 0] = 1
            got = check(ops, cuda, m)
            assert got[1].tolist() == [0, y, W - 1, y + 1, 2]


def _raw(lib, ops, fn, *args):
    return getattr(lib, fn)(*[ops._p(a) if torch.is_tensor(a) else a for a in args], ops._stream())


def test_output_is_owned_by_the_call(cuda):
    """garbage in `out` before the call, the call repeated on the same tensor, sentinels around it, and an input whose base is
    not 16-byte aligned (a view at a non-zero offset)"""
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    for (H, W), N in (((5, 7), 3), ((65, 63), 8), ((100, 130), 3)):
        m = random_masks(N, H, W, 0.2, seed=N + H)
        m[N // 2] = 0
        want = table(m)
        for off in (1, 3, 16, 21):
            base = torch.zeros(N * H * W + off, dtype=torch.uint8, device=cuda)
            view = base[off:].view(N, H, W)
            view.copy_(torch.from_numpy(m))
            assert view.data_ptr() % 16 == (base.data_ptr() + off) % 16
            buf = torch.full((N * 5 + 64,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
            out = buf[32:32 + N * 5]
            for _ in range(2):
                assert _raw(lib, ops, "vg_mask_boxes", view, out, N, H, W) == 0
                assert torch.equal(out.view(N, 5).cpu(), want)
            assert bool((buf[:32] == 0x5A5A5A5A).all()) and bool((buf[32 + N * 5:] == 0x5A5A5A5A).all())
            assert torch.equal(ops.mask_boxes(view).cpu(), want)
            # the filtered reduction owns its output in the same way
            ws = torch.empty((2, N, H, W), dtype=torch.int32, device=cuda)
            buf.fill_(0x5A5A5A5A)
            for _ in range(2):
                assert _raw(lib, ops, "vg_blob_boxes", view, out, None, ws[0], ws[1], N, H, W, 1) == 0
                assert torch.equal(out.view(N, 5).cpu(), want)                                # min_size 1 removes nothing
            assert bool((buf[:32] == 0x5A5A5A5A).all()) and bool((buf[32 + N * 5:] == 0x5A5A5A5A).all())


# ------------------------------------------------------------------------------------------------ mask_boxes(min_size)
def check_chain(ops, dm, min_size):
    """the fused entry point == mask_boxes(remove_small_blobs(.)), and its mask == remove_small_blobs(.)"""
    small = ops.remove_small_blobs(dm, min_size)
    want = ops.mask_boxes(small)
    assert torch.equal(ops.mask_boxes(dm, min_size), want)
    got, kept = ops.mask_boxes(dm, min_size, return_mask=True)
    assert torch.equal(got, want) and kept.dtype == torch.uint8 and torch.equal(kept, small)
    return want


@pytest.mark.parametrize("H,W", SHAPES)
def test_blob_boxes_against_the_two_calls(cuda, H, W):
    from videoglamm_amd import ops
    for N, d in ((1, 0.5), (3, 0.3), (8, 0.6), (3, 0.0), (1, 1.0), (3, 0.001)):
        m = random_masks(N, H, W, d, seed=H + 7 * W + N)
        dm = torch.from_numpy(m).to(cuda)
        for ms in (1, 2, 20, H * W, H * W + 1):
            want = check_chain(ops, dm, ms)
            if H * W <= 100 * 130:
                assert torch.equal(want.cpu(), torch.from_numpy(BR.boxes_np(m, ms)[0]))     # anchored in the numpy statement
    assert torch.equal(check_chain(ops, dm, 1), ops.mask_boxes(dm))


def test_blob_boxes_full_size(cuda):
    from oracle import postproc as OP
    from videoglamm_amd import ops
    m = OP.blobs((8, 1024, 1024), 3, density=0.4).astype(np.uint8)
    m |= random_masks(8, 1024, 1024, 0.001, seed=4)            # specks that the filter removes
    m[5] = 0
    dm = torch.from_numpy(m).to(cuda)
    want = check_chain(ops, dm, 20)
    assert not torch.equal(want, ops.mask_boxes(dm))


def test_blob_boxes_constructed(cuda):
    from videoglamm_amd import ops
    m = np.zeros((5, 150, 150), np.uint8)
    m[0, 3, 2:21] = 1                     # 19 pixels: removed at min_size 20
    m[0, 9, 30:50] = 1                    # 20 pixels: kept
    m[1, 60:70, 63] = 1                   # 10 + 10 pixels on the two sides of the tile border x = 63 | 64
    m[1, 60:70, 64] = 1
    m[1, 100:102, 100:105] = 1            # 10 pixels away from every border: removed
    m[2, 10, 10:140] = 1                  # a snake through all four 64 x 64 tiles of the first two tile rows / columns ...
    m[2, 10:140, 139] = 1
    m[2, 139, 70:140] = 1
    m[2, 0, 0] = 1                        # ... and a lone pixel
    m[3] = (np.add.outer(np.arange(150), np.arange(150)) % 2).astype(np.uint8)     # checkerboard: every component has area 1
    m[4, 63:65, 63:65] = 1                # 4 pixels, one in each of four tiles
    dm = torch.from_numpy(m).to(cuda)
    want = check_chain(ops, dm, 20)
    assert want[0].tolist() == [30, 9, 49, 9, 20]
    assert want[1].tolist() == [63, 60, 64, 69, 20]
    assert want[2].tolist() == [10, 10, 139, 139, 130 + 129 + 69]
    assert want[3].tolist() == want[4].tolist() == [150, 150, -1, -1, 0]
    assert torch.equal(want.cpu(), torch.from_numpy(BR.boxes_np(m, 20)[0]))
    assert check_chain(ops, dm, 1)[3].tolist() == [0, 0, 149, 149, 150 * 150 // 2]
    assert check_chain(ops, dm, 2)[3].tolist() == [150, 150, -1, -1, 0]
    assert check_chain(ops, dm, 4)[4].tolist() == [63, 63, 64, 64, 4] and check_chain(ops, dm, 5)[4].tolist() == [150, 150, -1, -1, 0]


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(cuda):
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    N, H, W = 2, 8, 9
    m = torch.ones((N, H, W), dtype=torch.uint8, device=cuda)
    ws = torch.empty((2, N, H, W), dtype=torch.int32, device=cuda)
    out = torch.full((N, 5), 77, dtype=torch.int32, device=cuda)
    bad = [("vg_mask_boxes", (None, out, N, H, W)), ("vg_mask_boxes", (m, None, N, H, W)), ("vg_mask_boxes", (m, out, 0, H, W)),
           ("vg_mask_boxes", (m, out, N, 0, W)), ("vg_mask_boxes", (m, out, N, 1 << 16, 1 << 15)),
           ("vg_blob_boxes", (None, out, None, ws[0], ws[1], N, H, W, 20)), ("vg_blob_boxes", (m, None, None, ws[0], ws[1], N, H, W, 20)),
           ("vg_blob_boxes", (m, out, None, None, ws[1], N, H, W, 20)), ("vg_blob_boxes", (m, out, None, ws[0], ws[1], 0, H, W, 20)),
           ("vg_blob_boxes", (m, out, None, ws[0], ws[1], N, H, W, 0)), ("vg_blob_boxes", (m, out, None, ws[0], ws[1], N, H, W, -3))]
    for fn, args in bad:
        assert _raw(lib, ops, fn, *args) != 0, (fn, args)
        assert fn.encode() in lib.vg_last_error()
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                   # nothing was launched
    with pytest.raises(_lib.VGKernelError, match="vg_mask_boxes"):
        ops.mask_boxes(torch.ones((0, 4, 4), dtype=torch.uint8, device=cuda))
    assert ops.mask_boxes(m, 0).tolist() == [[0, 0, W - 1, H - 1, H * W]] * N      # min_size 0 is routed to vg_mask_boxes


# ------------------------------------------------------------------------------------------------ the reference's outputs
def test_masks_to_boxes_against_reference(cuda):
    from videoglamm_amd import postproc as PP
    g = G.fixture("grounding.npz")
    for m in (g["masks"].to(cuda), g["masks"].bool().to(cuda), g["masks"].numpy(), g["masks"].numpy().astype(bool)):
        out = PP.masks_to_boxes(m)
        assert out.is_cuda and out.dtype == torch.float32 and torch.equal(out.cpu(), g["boxes"])
    out = PP.masks_to_boxes(torch.zeros((0, 8, 8), dtype=torch.bool, device=cuda))
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (0, 4)
    assert torch.equal(PP.masks_to_boxes(g["masks"].to(cuda), min_size=20).cpu(), torch.from_numpy(BR.xyxy_np(g["masks"].numpy(), 20)))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def micro(cuda):
    import test_clips_gpu as TC
    return TC._micro(cuda)


def check_twin(ref, got):
    """got = (ids, [segments], [boxes]) of a return_boxes call, ref = the plain call's pair: same ids, same masks, and the boxes
    are the statement's on the returned masks"""
    assert len(ref) == 2 and len(got) == 3 and torch.equal(got[0], ref[0])
    assert len(got[1]) == len(got[2]) == len(ref[1]) == 1
    seg, rseg, box = got[1][0], ref[1][0], got[2][0]
    assert list(seg) == list(rseg) == list(box)
    for t in seg:
        assert list(seg[t]) == list(rseg[t]) == list(box[t])
        for k in seg[t]:
            assert np.array_equal(seg[t][k], rseg[t][k])
            b = box[t][k]
            assert isinstance(b, np.ndarray) and b.dtype == np.float32 and b.shape == (4,)
            assert np.array_equal(b, BR.xyxy_np(seg[t][k])), (t, k)
    return len(seg)


@pytest.mark.parametrize("blob", [0, 20])
@pytest.mark.parametrize("video", [False, True])
def test_inference_return_boxes(micro, video, blob, monkeypatch):
    m, clips = micro
    monkeypatch.setattr(m, "min_blob_size", blob)
    kw = dict(max_new_tokens=8, use_sam2_video_branch=video)
    ref = m.inference(*clips[0], **kw)
    assert check_twin(ref, m.inference(*clips[0], return_boxes=True, **kw)) == 3
    assert len(m.inference(*clips[0], **kw)) == 2


@pytest.mark.parametrize("video", [False, True])
def test_clips_and_prompts_return_boxes(micro, video, monkeypatch):
    m, clips = micro
    monkeypatch.setattr(m, "min_blob_size", 20 if video else 0)
    kw = dict(max_new_tokens=8, use_sam2_video_branch=video)
    ref = m.inference_clips(clips[:2], **kw)
    got = m.inference_clips(clips[:2], return_boxes=True, **kw)
    assert len(ref) == len(got) == 2
    for r, g in zip(ref, got):
        check_twin(r, g)
    images, context, sam, ids, resize, hw = clips[0]
    n0 = int((ids[0] == -200).nonzero().max()) + 1
    prompts = [ids[0], torch.cat([ids[0][:n0], torch.tensor([84, 12, 99, 150, 7])])]
    ref = m.inference_prompts(images, context, sam, prompts, resize, hw, **kw)
    got = m.inference_prompts(images, context, sam, prompts, resize, hw, return_boxes=True, **kw)
    assert len(ref) == 2 and len(got) == 3 and len(got[0]) == len(got[1]) == len(got[2]) == 2
    for b in range(2):
        check_twin((ref[0][b], [ref[1][b]]), (got[0][b], [got[1][b]], [got[2][b]]))
