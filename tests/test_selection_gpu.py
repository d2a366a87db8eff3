"""The kernels that make discrete decisions, on the MI355X (-m gpu): which token is emitted (vg_argmax, vg_argmax_partial + vg_decode_step_end
and their _rows forms, vg_token_scores_rows' top1, the sampler at signed zeros), which mask SAM2 keeps (vg_multimask_select) and which side of
zero a value is on (vg_threshold, vg_where_rows, vg_mask_for_mem).  Every comparison is exact: an index, a bit pattern or torch.equal.  The
cases come from tests/_select_ref.py; tests/test_selection_selfcheck.py shows that a wrong kernel cannot pass them."""
import numpy as np
import pytest
import torch

import _cpu_ops as ref
import _cpu_sampling as S
import _select_ref as R

torch.set_grad_enabled(False)

pytestmark = pytest.mark.gpu

SENT = -77
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
STEP_NS = (2049, 32064, 128256, 131073)


def _dev(x, dt, cuda):
    """a case's rows on the device in the dtype under test (the values are representable: the cast is exact)"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DTYPES[dt])
    assert np.array_equal(t.float().numpy().view(np.uint32), np.ascontiguousarray(x).view(np.uint32))
    return t.to(cuda)


def _guarded(n, cuda, dtype=torch.int64, fill=SENT, zero=False):
    """(buffer [n + 2] with a sentinel at either end, its middle n entries)"""
    buf = torch.full((n + 2,), fill, dtype=dtype, device=cuda)
    if zero:
        buf[1:n + 1] = 0
    return buf, buf[1:n + 1]


def _token(acc):
    """the index in packed (ordered value bits, ~index) keys"""
    return [0xFFFFFFFF - (int(a) & 0xFFFFFFFF) for a in acc.tolist()]


# ---- vg_argmax -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n,name", [(n, name) for n in R.NS for name in R.case_names(n)], ids=lambda v: str(v))
def test_argmax_one_row(cuda, n, name, dt):
    from videoglamm_amd import ops
    row, want = R.build_case(n, name, dt == "bf16")
    buf, out = _guarded(1, cuda)
    ops.argmax(_dev(row[None], dt, cuda), out=out)
    assert buf.tolist() == [SENT, want, SENT]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("rows", [3, 16])
@pytest.mark.parametrize("n", R.NS)
def test_argmax_packed_rows(cuda, n, rows, dt):
    """[rows, n] calls whose rows are different cases of the same n, until every case has been a row: row indexing, and with odd n in bf16
    rows that start off a dword"""
    from videoglamm_amd import ops
    for start in range(0, len(R.case_names(n)), rows):
        names, x, want = R.pack(n, rows, dt == "bf16", start)
        buf, out = _guarded(rows, cuda)
        ops.argmax(_dev(x, dt, cuda), out=out)
        got = buf.tolist()
        assert got[0] == SENT == got[-1]
        assert got[1:-1] == want.tolist(), [nm for nm, g, w in zip(names, got[1:-1], want) if g != w]


# ---- vg_argmax_partial(_rows) + vg_decode_step_end(_rows) ----------------------------------------------------------------------------------
def _step_state(B, cuda, D=64, max_len=8, cap=4):
    st = dict(tok=torch.full((B,), 17, dtype=torch.int64), pos=torch.tensor([b % 5 for b in range(B)], dtype=torch.int32),
              step=torch.zeros(B, dtype=torch.int32), forced=torch.tensor([[-1, 1000 + b, -1] for b in range(B)], dtype=torch.int64),
              hist=torch.full((B, cap), SENT, dtype=torch.int64), raw=torch.full((B, cap), SENT, dtype=torch.int64),
              hid=torch.zeros(B, max_len, D, dtype=torch.bfloat16))
    return st, {k: v.to(cuda) for k, v in st.items()}


def _step_end_cpu(st, picks, rows):
    """vg_decode_step_end's statement (include/vg_kernels.h) on the host copy of the state"""
    for b, t0 in enumerate(picks):
        k, p = int(st["step"][b]), int(st["pos"][b])
        st["hid"][b, p] = rows[b]
        f = int(st["forced"][b, k]) if k < st["forced"].shape[1] else -1
        st["raw"][b, k] = t0
        st["tok"][b] = f if f >= 0 else t0
        st["hist"][b, k] = st["tok"][b]
        st["step"][b] = k + 1
        st["pos"][b] = p + 1


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("form,B", [("single", 1), ("rows", 1), ("rows", 5), ("rows", 16)])
@pytest.mark.parametrize("n", STEP_NS)
def test_argmax_partial_and_step_end(cuda, n, B, form, dt):
    """every case of row length n through the two launches of a decode step's tail, B cases per round, rounds of three on one state and ALL
    rounds on one accumulator (the single-row launches with B = 1, the _rows launches with B = 1, 5, 16): the emitted token and raw[] are
    the reference index, a forced id (round 1) overrides tok / hist but not raw, pos / step advance, the hidden row lands in slot pos of its
    own batch row and nowhere else, the accumulator is left zero."""
    from videoglamm_amd import ops
    ncases = len(R.case_names(n))
    accbuf, acc = _guarded(B, cuda, zero=True)
    g = torch.Generator().manual_seed(n + B)
    rnd = 0
    for start in range(0, max(ncases, 3 * B), B):
        if rnd % 3 == 0:
            st, d = _step_state(B, cuda)
        names, x, want = R.pack(n, B, dt == "bf16", start)
        xd = _dev(x, dt, cuda)
        hrow = torch.randn(B, 64, generator=g).to(torch.bfloat16)
        if form == "single":
            ops.argmax_partial(xd.view(-1), acc)
        else:
            ops.argmax_partial_rows(xd, acc)
        picks = _token(acc)
        assert picks == want.tolist(), [nm for nm, p, w in zip(names, picks, want) if p != w]
        if form == "single":
            ops.decode_step_end(acc, d["tok"], d["pos"], d["step"], hrow.to(cuda), d["hid"][0], d["forced"][0], d["hist"][0], d["raw"][0])
        else:
            ops.decode_step_end_rows(acc, d["tok"], d["pos"], d["step"], hrow.to(cuda), d["hid"], d["forced"], d["hist"], d["raw"])
        _step_end_cpu(st, want.tolist(), hrow)
        assert accbuf.tolist() == [SENT] + [0] * B + [SENT]
        for k in st:
            assert torch.equal(d[k].cpu(), st[k]), (k, rnd, names)
        rnd += 1
    assert rnd >= 3 and int(st["step"][0]) == (rnd - 1) % 3 + 1


# ---- agreement with vg_token_scores_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", STEP_NS)
def test_scores_top1_is_the_argmax_token_on_ties_and_signed_zeros(cuda, n):
    """on every tie and signed-zero row: vg_token_scores_rows' top1 is the token vg_argmax_partial's key names, the reference index, and the
    top-2 margin is exactly 0 (top2 holds the same value)"""
    from videoglamm_amd import ops
    names = [nm for nm in R.case_names(n) if nm.startswith(("tie_", "zeros_"))]
    assert len(names) >= 15
    cap = 4
    for s in range(0, len(names), 16):
        chunk = names[s:s + 16]
        built = [R.build_case(n, nm, False) for nm in chunk]
        B = len(chunk)
        x = torch.from_numpy(np.stack([r for r, _ in built])).to(cuda)
        want = [w for _, w in built]
        acc = torch.zeros(B, dtype=torch.int64, device=cuda)
        ops.argmax_partial_rows(x, acc)
        step = torch.tensor([b % cap for b in range(B)], dtype=torch.int32, device=cuda)
        scores = torch.full((B, cap, 2), 777.0, dtype=torch.float32, device=cuda)
        top2 = torch.full((B, cap, 2), SENT, dtype=torch.int64, device=cuda)
        ops.token_scores_rows(x, step, scores, top2, acc=acc, ws=ops.token_scores_workspace(B, cuda))
        bi = torch.arange(B)
        top1 = top2.cpu()[bi, step.cpu().long(), 0].tolist()
        margin = scores.cpu()[bi, step.cpu().long(), 1]
        assert _token(acc) == want == top1, [nm for nm, a, w, t in zip(chunk, _token(acc), want, top1) if not a == w == t]
        assert torch.equal(margin, torch.zeros(B)), [nm for nm, m in zip(chunk, margin.tolist()) if m != 0]


# ---- vg_multimask_select -------------------------------------------------------------------------------------------------------------------
HW_SHAPES = {50: (5, 10), 63: (7, 9), 400: (20, 20), 4100: (50, 82), 65536: (256, 256)}


def _multimask_guarded(masks, ious, tokens, mode, cuda):
    """ops.multimask_select's call with the output mask inside a sentinel-filled buffer (16-byte aligned, as the wrapper's own is)
    -> (mask, iou, token, idx, the buffer's guard entries)"""
    from videoglamm_amd import _lib, ops
    N, _, h, w = masks.shape
    C = tokens.shape[-1]
    buf = torch.full((N * h * w + 8,), float(SENT), dtype=torch.float32, device=cuda)
    om = buf[4:4 + N * h * w].view(N, 1, h, w)
    oi = torch.empty(N, dtype=torch.float32, device=cuda)
    ot = torch.empty(N, C, dtype=tokens.dtype, device=cuda)
    ox = torch.empty(N, dtype=torch.int32, device=cuda)
    assert om.data_ptr() % 16 == 0 and masks.is_contiguous()
    rc = _lib.load().vg_multimask_select(ops._p(masks), ops._p(ious), ops._p(tokens), ops._p(om), ops._p(oi), ops._p(ot), ops._p(ox), N, h * w, C,
                                         0.05, 0.98, int(mode), ops._dt(tokens), ops._stream())
    _lib.check(rc, "vg_multimask_select")
    return om, oi, ot, ox, torch.cat([buf[:4], buf[-4:]])


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("HW", R.HWS)
def test_multimask_select_on_and_around_the_thresholds(cuda, HW, offset):
    """every IoU row of the best-of-3 rule with token-0 masks whose stability score sits on the threshold, one pixel under it, on the empty
    mask and on the full one, pixels exactly on +-delta included; on a 16-byte aligned buffer and on one offset by a float (still contiguous:
    the scalar route at HW % 4 == 0, the one-workgroup kernel in mode 1)"""
    from videoglamm_amd import ops
    names, masks, ious, best, stable = R.selection_cases(HW)
    N, (h, w) = len(names), HW_SHAPES[HW]
    m_cpu = torch.from_numpy(masks).view(N, 4, h, w)
    i_cpu = torch.from_numpy(ious)
    t_cpu = torch.randn(N, 4, 256, generator=torch.Generator().manual_seed(HW)).to(torch.bfloat16)
    flat = torch.zeros(N * 4 * HW + 4, dtype=torch.float32, device=cuda)
    m_dev = flat[offset:offset + N * 4 * HW].view(N, 4, h, w)
    m_dev.copy_(m_cpu)
    assert m_dev.is_contiguous() and m_dev.data_ptr() % 16 == 4 * offset
    for mode in (0, 1):
        wm, wi, wt, wx = R.multimask_select(m_cpu, i_cpu, t_cpu, mode)
        assert wx.tolist() == (np.where(stable, 0, best) if mode == 0 else best).tolist()
        om, oi, ot, ox, guard = _multimask_guarded(m_dev, i_cpu.to(cuda), t_cpu.to(cuda), mode, cuda)
        bad = [nm for nm, g, e in zip(names, ox.tolist(), wx.tolist()) if g != e]
        assert not bad, (mode, bad)
        assert torch.equal(om.cpu(), wm) and torch.equal(oi.cpu(), wi) and torch.equal(ot.cpu(), wt) and torch.equal(ox.cpu(), wx), mode
        assert torch.equal(guard.cpu(), torch.full((8,), float(SENT)))
        for g, e in zip(ops.multimask_select(m_dev, i_cpu.to(cuda), t_cpu.to(cuda), mode), (wm, wi, wt, wx)):        # the wrapper, same view
            assert torch.equal(g.cpu(), e), mode


# ---- the strict > 0 deciders ---------------------------------------------------------------------------------------------------------------
N_PW = 2 ** 20 + 3          # past the 2^20 entries at which the pointwise grid stops growing: the grid-stride loop runs


def test_threshold_specials(cuda):
    from videoglamm_amd import ops
    x, pos = R.specials_in_noise(N_PW, 1)
    got = ops.threshold(torch.from_numpy(x).to(cuda)).cpu()
    assert got.dtype == torch.uint8 and torch.equal(got, (torch.from_numpy(x) > 0).to(torch.uint8))
    assert got[torch.from_numpy(pos)].tolist() == np.tile(R.SPECIALS_POSITIVE, 5).astype(int).tolist()


@pytest.mark.parametrize("out_dt", list(DTYPES))
def test_mask_for_mem_binarize_specials(cuda, out_dt):
    from videoglamm_amd import ops
    x, pos = R.specials_in_noise(N_PW, 2)
    got = ops.mask_for_mem(torch.from_numpy(x).to(cuda), True, 20.0, -10.0, DTYPES[out_dt]).cpu()
    assert torch.equal(got, ref.mask_for_mem(torch.from_numpy(x), True, 20.0, -10.0, DTYPES[out_dt]))
    assert got[torch.from_numpy(pos)].float().tolist() == np.where(np.tile(R.SPECIALS_POSITIVE, 5), 10.0, -10.0).tolist()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("form", ["fill", "b"])
def test_where_rows_specials(cuda, dt, form):
    """cond = the specials, one row each; rows * inner just past 2^20; the destination a strided row view whose gaps stay untouched"""
    from videoglamm_amd import ops
    rows = len(R.SPECIALS)
    inner = -(-(2 ** 20 + 1) // rows)
    assert 2 ** 20 < rows * inner < 2 ** 20 + 2 * rows
    g = torch.Generator().manual_seed(5)
    a = torch.randn(rows, inner, generator=g).to(DTYPES[dt])
    b = torch.randn(inner, generator=g).to(DTYPES[dt]) if form == "b" else None
    cond = torch.from_numpy(R.SPECIALS)
    buf = torch.full((rows, inner + 8), float(SENT), dtype=DTYPES[dt], device=cuda)
    out = buf[:, :inner]
    ops.where_rows(cond.to(cuda), a.to(cuda), None if b is None else b.to(cuda), fill=-7.5, out=out)
    keep = torch.from_numpy(R.SPECIALS_POSITIVE)[:, None]
    want = torch.where(keep, a, b[None, :].expand_as(a) if b is not None else torch.full_like(a, -7.5))
    got = buf.cpu()
    assert torch.equal(got[:, :inner], want), [i for i in range(rows) if not torch.equal(got[i, :inner], want[i])]
    assert torch.equal(got[:, :inner], ref.where_rows(cond, a, b, fill=-7.5))
    assert torch.equal(got[:, inner:], torch.full((rows, 8), float(SENT), dtype=DTYPES[dt]))


# ---- the sampler at signed zeros -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("plus_at", [1, 2], ids=["plus_zero_middle", "plus_zero_last"])
@pytest.mark.parametrize("n", [4100, 32064])
def test_sampler_keeps_and_walks_signed_zeros_as_equal(cuda, n, plus_at, k):
    """a row of -1 with one +0.0 and two -0.0, each in another slice of the fast route: HF's float comparisons keep all three under top-k
    (k = 1 and 2: ties at the threshold are kept), 1/3 each — fp32(1) * (fp32(1) / fp32(3)) in the kernel's arithmetic, the float64 third
    rounded to fp32 in the reference: the same number — and the draw walks them by ascending index, on both routes"""
    from videoglamm_amd import ops
    nb = -(-n // 2048)
    chunk = -(-n // nb)
    at = [5, chunk + 700, 2 * chunk + 11]
    assert len({i // chunk for i in at}) == 3 and at[-1] < n
    x = np.full(n, -1.0, np.float32)
    x[at] = -0.0
    x[at[plus_at]] = 0.0
    order, prob, _ = S.kept(x, 1.0, k, 1.0)
    assert order.tolist() == at and prob.tolist() == [1 / 3] * 3
    xd = torch.from_numpy(x).to(cuda)
    params = ops.sampling_params(1.0, k, 1.0, 0, cuda)
    idx, pr = ops.sample_survivors(xd, params)
    assert idx.tolist() == at
    assert torch.equal(pr, torch.tensor(prob, dtype=torch.float64).to(torch.float32))
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    ws = ops.sample_workspace(cuda)
    assert ops.sample_fast_route(k, n)
    for u in (1 / 6, 1 / 2, 5 / 6):
        want, _ = S.draw(order, prob, u)
        assert want == at[int(3 * u)]
        u_dev = torch.tensor([u], dtype=torch.float32, device=cuda)
        for fast in (None, ws):
            acc = torch.zeros(1, dtype=torch.int64, device=cuda)
            tok = torch.full((1,), SENT, dtype=torch.int64, device=cuda)
            ops.sample_partial(xd, params, step, acc=acc, tok=tok, u_override=u_dev, fast_ws=fast)
            assert _token(acc) == tok.tolist() == [want], ("general" if fast is None else "fast", u)
    assert int(ws[-64]) == 0
