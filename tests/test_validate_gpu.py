"""Validation class counts on the MI355X (vg_logit_class_counts; ops.logit_class_counts, postproc.intersectionAndUnionGPU /
validation_record, model.validate).  Integer counts, so every check is torch.equal: against the numpy statement of the contract
(tests/_validate_ref.py), against the reference's own outputs (tests/golden/validate.npz), and end to end on the tiny model."""
import numpy as np
import pytest
import torch

import _validate_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.0, -1.0], np.float32)


def random_case(N, H, W, seed):
    """logits float32 [N, H, W] (normal values, exact zeros and the special values mixed in), target uint8 [N, H, W] of
    0 / 1 / 255 and a few stray labels"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, H, W)).astype(np.float32)
    pick = rng.random((N, H, W))
    x = np.where(pick < 0.1, SPECIAL[rng.integers(0, len(SPECIAL), size=(N, H, W))], x).astype(np.float32)
    t = rng.choice(np.array([0, 1, 255, 7, 254, 2], np.uint8), size=(N, H, W), p=[0.45, 0.35, 0.15, 0.02, 0.02, 0.01])
    return x, t


def at_offset(a, off, device):
    """a device copy of `a` whose first element lies `off` elements behind an allocation's start"""
    src = a if torch.is_tensor(a) else torch.from_numpy(a)
    base = torch.zeros(src.numel() + off, dtype=src.dtype, device=device)
    view = base[off:].view(src.shape)
    view.copy_(src)
    assert view.is_contiguous() and view.data_ptr() == base.data_ptr() + off * src.element_size()
    return view


def _raw(lib, ops, *args):
    return lib.vg_logit_class_counts(*[ops._p(a) if torch.is_tensor(a) else a for a in args], ops._stream())


# ------------------------------------------------------------------------------------------------ kernel against the statement
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(1, 1), (37, 53), (64, 64), (360, 640)])
@pytest.mark.parametrize("N", [1, 3, 30])
def test_counts_against_statement(cuda, N, H, W, dtype):
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    x, t = random_case(N, H, W, seed=N * 7919 + H * 31 + W)
    xs = torch.from_numpy(x).to(dtype)                               # the comparison is on the STORED value: the statement gets it
    with np.errstate(invalid="ignore"):
        want = torch.from_numpy(R.counts(xs.float().numpy(), t, 255))
    got = ops.logit_class_counts(xs.to(cuda), torch.from_numpy(t).to(cuda))
    assert got.dtype == torch.int64 and tuple(got.shape) == (N, 6) and torch.equal(got.cpu(), want)
    # rows that start at an odd element, `out` full of garbage, sentinels around it, the call repeated
    dx, dt = at_offset(xs, 1, cuda), at_offset(t, 3, cuda)
    assert dx.data_ptr() % 16 != 0 and dt.data_ptr() % 16 != 0
    buf = torch.full((N * 6 + 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=cuda)
    out = buf[32:32 + N * 6]
    first = None
    for _ in range(2):
        assert _raw(lib, ops, dx, dt, out, N, H * W, ops._dt(dx), 255) == 0
        assert torch.equal(out.view(N, 6).cpu(), want)
        first = out.clone() if first is None else first
    assert torch.equal(first, out)
    assert bool((buf[:32] == 0x5A5A5A5A5A5A5A5A).all()) and bool((buf[32 + N * 6:] == 0x5A5A5A5A5A5A5A5A).all())
    assert torch.equal(ops.logit_class_counts(dx, dt).cpu(), want)


@pytest.mark.parametrize("ignore_index", [0, 1, 7, 254])
def test_other_ignore_labels(cuda, ignore_index):
    from videoglamm_amd import ops
    x, t = random_case(3, 37, 53, seed=5)
    with np.errstate(invalid="ignore"):
        want = torch.from_numpy(R.counts(x, t, ignore_index))
    assert torch.equal(ops.logit_class_counts(torch.from_numpy(x).to(cuda), torch.from_numpy(t).to(cuda), ignore_index).cpu(), want)


def test_every_head_and_tail_length(cuda):
    """L and the row start run through every residue of the 16-pixel groups and of the 16-byte boundary, with more than one
    workgroup's worth of groups in between for the longer rows"""
    from videoglamm_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        for L in list(range(1, 40)) + [16 * 1024 * 3 + 5]:
            x, t = random_case(2, 1, L, seed=L)
            xs = torch.from_numpy(x).to(dtype)
            with np.errstate(invalid="ignore"):
                want = torch.from_numpy(R.counts(xs.float().numpy(), t, 255))
            for off in ((0, 0), (1, 0), (2, 5), (3, 15), (5, 8), (7, 1)) if L < 40 else ((3, 5),):
                got = ops.logit_class_counts(at_offset(xs, off[0], cuda), at_offset(t, off[1], cuda))
                assert torch.equal(got.cpu(), want), (dtype, L, off)


def test_large_count_is_exact(cuda):
    """one mask of 2^24 + 3 pixels, every logit positive, every target 1: a float32 accumulator would lose the 3"""
    from videoglamm_amd import ops
    L = 2 ** 24 + 3
    x = torch.full((1, 1, L), 0.5, dtype=torch.float32, device=cuda)
    t = torch.ones((1, 1, L), dtype=torch.uint8, device=cuda)
    assert float(torch.tensor(float(L), dtype=torch.float32)) != L
    assert ops.logit_class_counts(x, t).tolist() == [[0, L, 0, L, 0, L]]
    assert ops.logit_class_counts(x.to(torch.bfloat16), t).tolist() == [[0, L, 0, L, 0, L]]


def test_pixel_indices_past_2_to_31(cuda):
    """two bf16 masks of 2^30 + 5 pixels: the second one's pixels lie past element 2^31 of both inputs"""
    from videoglamm_amd import ops
    L = 2 ** 30 + 5
    x = torch.ones((2, 1, L), dtype=torch.bfloat16, device=cuda)
    t = torch.zeros((2, 1, L), dtype=torch.uint8, device=cuda)
    x[1, 0, -7:] = -1.0
    t[1, 0, -3:] = 1
    t[1, 0, 0] = 255
    t[1, 0, L // 2] = 255
    # mask 0: all class 1 on target 0.  mask 1: L - 2 live pixels, 7 of class 0 (the last 7), targets: 3 ones among them
    want = [[0, 0, 0, L, L, 0], [4, 0, 7, L - 2 - 7, L - 2 - 3, 3]]
    assert ops.logit_class_counts(x, t).tolist() == want


def test_special_values_fall_on_the_right_side(cuda):
    from videoglamm_amd import ops
    fx = R.fixture()
    ign = int(fx["ignore_index"])
    for name in ("s0", "s1", "s2", "one"):
        x, t = torch.from_numpy(fx[f"{name}_logits"]), torch.from_numpy(fx[f"{name}_target"])
        for dtype in (torch.float32, torch.bfloat16):
            xs = x.to(dtype)
            with np.errstate(invalid="ignore"):
                want = torch.from_numpy(R.counts(xs.float().numpy(), t.numpy(), ign))
            assert torch.equal(ops.logit_class_counts(xs.to(cuda), t.to(cuda), ign).cpu(), want), (name, dtype)
        inter, union, tgt = R.triples(ops.logit_class_counts(x.to(cuda), t.to(cuda), ign).cpu().numpy())
        assert np.array_equal(np.stack([inter, union, tgt], 1), fx[f"{name}_triples"])           # fp32: the reference's own triples
    # bit patterns, one pixel per mask, target 1: out1 says which side the value fell on
    f32 = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0xff800000,
                    0x7f800001, 0x7fc00000, 0xffc00000, 0xffffffff, 0x3f800000, 0xbf800000], np.uint32)
    b16 = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x0080, 0x7f7f, 0x7f80, 0xff80, 0x7f81, 0x7fc0, 0xffc0, 0xffff, 0x3f80, 0xbf80], np.uint16)
    pos = [0, 0, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0]
    ones = torch.ones((len(pos), 1, 1), dtype=torch.uint8, device=cuda)
    for bits, view in ((f32.view(np.int32), torch.float32), (b16.view(np.int16), torch.bfloat16)):
        x = torch.from_numpy(bits.copy()).view(view).reshape(-1, 1, 1).to(cuda)
        assert ops.logit_class_counts(x, ones)[:, 3].tolist() == pos, view
    with np.errstate(invalid="ignore"):
        assert (f32.view(np.float32) > 0).astype(int).tolist() == pos


# ------------------------------------------------------------------------------------------------ the operator's surface
def test_operator_surface(cuda):
    from videoglamm_amd import ops
    x, t = random_case(6, 9, 11, seed=3)
    t = np.where(t > 1, 255, t).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        want = torch.from_numpy(R.counts(x, t, 255))
    dx = torch.from_numpy(x).to(cuda)
    for tt in (torch.from_numpy(t), torch.from_numpy(t).int(), torch.from_numpy(t).long(), torch.from_numpy(t).to(torch.int16)):
        assert torch.equal(ops.logit_class_counts(dx, tt.to(cuda)).cpu(), want)
    got = ops.logit_class_counts(dx.view(2, 3, 9, 11), torch.from_numpy(t).to(cuda).view(2, 3, 9, 11))      # leading dimensions are kept
    assert tuple(got.shape) == (2, 3, 6) and torch.equal(got.view(6, 6).cpu(), want)
    tb = torch.from_numpy(t == 1)                                                                         # bool: labels 0 / 1
    with np.errstate(invalid="ignore"):
        assert torch.equal(ops.logit_class_counts(dx, tb.to(cuda)).cpu(), torch.from_numpy(R.counts(x, tb.numpy().astype(np.uint8), 255)))
    for bad in (256, -1):
        tt = torch.from_numpy(t).int()
        tt[0, 0, 0] = bad
        with pytest.raises(AssertionError, match="0..255"):
            ops.logit_class_counts(dx, tt.to(cuda))
    with pytest.raises(AssertionError):
        ops.logit_class_counts(dx, torch.from_numpy(t).float().to(cuda))
    with pytest.raises(AssertionError):
        ops.logit_class_counts(dx, torch.from_numpy(t).to(cuda)[:, :, :10])
    with pytest.raises(AssertionError):
        ops.logit_class_counts(dx.double(), torch.from_numpy(t).to(cuda))


def test_argument_errors(cuda):
    from videoglamm_amd import _lib, ops
    lib = _lib.load()
    N, L = 2, 72
    x = torch.ones((N, L), dtype=torch.float32, device=cuda)
    t = torch.ones((N, L), dtype=torch.uint8, device=cuda)
    buf = torch.full((N * 6 + 64,), 77, dtype=torch.int64, device=cuda)
    out = buf[32:32 + N * 6]
    F32, BF16 = ops._dt(x), ops._dt(x.to(torch.bfloat16))
    bad = [(None, t, out, N, L, F32, 255), (x, None, out, N, L, F32, 255), (x, t, None, N, L, F32, 255), (x, t, out, 0, L, F32, 255),
           (x, t, out, -1, L, F32, 255), (x, t, out, 65536, L, F32, 255), (x, t, out, N, 0, F32, 255), (x, t, out, N, -5, F32, 255),
           (x, t, out, N, L, 2, 255), (x, t, out, N, L, -1, 255), (x, t, out, N, L, F32, -1), (x, t, out, N, L, BF16, 256)]
    for args in bad:
        assert _raw(lib, ops, *args) == -1, args                     # VG_ERR_ARG
        assert b"vg_logit_class_counts" in lib.vg_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 77).all())                                   # nothing was launched, nothing was cleared
    assert _raw(lib, ops, x, t, out, N, L, F32, 255) == 0
    assert out.view(N, 6).tolist() == [[0, L, 0, L, 0, L]] * N and bool((buf[:32] == 77).all()) and bool((buf[32 + N * 6:] == 77).all())
    with pytest.raises(_lib.VGKernelError, match="vg_logit_class_counts"):
        ops.logit_class_counts(torch.ones((0, 4, 4), device=cuda), torch.ones((0, 4, 4), dtype=torch.uint8, device=cuda))


# ------------------------------------------------------------------------------------------------ the reference's name and outputs
def test_intersection_and_union_against_reference(cuda):
    from videoglamm_amd import postproc as PP
    fx = R.fixture()
    ign = int(fx["ignore_index"])
    for name in ("s0", "s1", "s2", "one"):
        x, t = fx[f"{name}_logits"], fx[f"{name}_target"]
        with np.errstate(invalid="ignore"):
            labels = (x > 0).astype(np.float32)
        for f in range(x.shape[0]):
            want = torch.from_numpy(fx[f"{name}_triples"][f].astype(np.float32))
            for out, tgt in ((torch.from_numpy(labels[f]).to(cuda), torch.from_numpy(t[f]).float().to(cuda)),
                             (torch.from_numpy(labels[f]).int().to(cuda), torch.from_numpy(t[f]).int().to(cuda)), (labels[f], t[f])):
                before = out.clone() if torch.is_tensor(out) else out.copy()
                got = PP.intersectionAndUnionGPU(out, tgt, 2, ignore_index=ign)
                assert all(g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (2,) for g in got)
                assert torch.equal(torch.stack(got).cpu(), want), (name, f)
                assert torch.equal(out, before) if torch.is_tensor(out) else np.array_equal(out, before)
    # three dimensions in one call: the counts of all frames together
    x, t = fx["s2_logits"], fx["s2_target"]
    with np.errstate(invalid="ignore"):
        got = PP.intersectionAndUnionGPU(torch.from_numpy((x > 0).astype(np.float32)).to(cuda), torch.from_numpy(t).to(cuda), 2, ign)
    assert torch.equal(torch.stack(got).cpu(), torch.from_numpy(fx["s2_triples"].sum(0).astype(np.float32)))


def test_validation_record_against_reference(cuda):
    from videoglamm_amd import postproc as PP
    fx = R.fixture()
    ign = int(fx["ignore_index"])
    meter = PP.ValidationMeter()
    for s in range(3):
        x, t = R.sample_frames(fx, s)
        out = {"pred_masks": [[torch.from_numpy(x[f])[None].to(cuda) for f in range(x.shape[0])]], "gt_masks": [torch.from_numpy(t)[None].to(cuda)]}
        rec = PP.validation_record(out, ign)
        for got, key in zip(rec[:3], ("intersection", "union", "acc_iou")):
            assert got.dtype == np.float32 and got.tobytes() == fx[f"s{s}_{key}"].tobytes(), (s, key)
        assert rec[3] == x.shape[0]
        meter.update(rec)
        counts = PP.validation_counts(torch.from_numpy(x).to(cuda), torch.from_numpy(t).int().to(cuda), ign)      # [T, H, W], integer labels
        with np.errstate(invalid="ignore"):
            assert tuple(counts.shape) == (x.shape[0], 6) and torch.equal(counts.cpu(), torch.from_numpy(R.counts(x, t, ign)))
    giou, ciou = meter.result()
    assert giou == float(fx["giou"]) and ciou == float(fx["ciou"])


# ------------------------------------------------------------------------------------------------ end to end
def test_validate_end_to_end(cuda):
    """the tiny synthetic model of tests/test_facade.py: model_forward(inference=True) with a ground truth that carries an ignore
    band -> validation_record == the host arithmetic on the statement's counts of the downloaded logits; validate() over two
    samples == the meter fed by hand"""
    from test_validate import check_validate_end_to_end

    check_validate_end_to_end(cuda)
