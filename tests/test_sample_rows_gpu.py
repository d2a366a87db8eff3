"""The B-row sampling launch (vg_sample_partial_rows): every row of a batched decode step drawn in ONE launch, bit-identical to vg_sample_partial
on that row alone (the same packed key in acc[b], the same tok[b]) with the row's own parameter block, step word, uniform and workspace."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _logits(B, V, seed, pad=0):
    """[B, V] fp32 rows of a [B, V + pad] tensor (pad > 0: a row stride longer than the row)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V + pad, generator=g) * 2.5
    return x


def _tie_block(x, ties, k, at=1000):
    """`ties` equal values directly under the 30th largest of the row x (the next float below it), all in the first fast-route slice (indices
    at .. at + ties).  With 30 < k <= 30 + ties the global k-th value is the tied one and that slice holds more than 64 of them: the slice keeps
    64, flags the rest, and the row's last workgroup must run the general route (the fast route's tie overflow).  The construction is checked
    here on the host, so another seed cannot disarm the test."""
    V = x.numel()
    top = torch.topk(x, 30).values
    tied = torch.nextafter(top[-1], torch.tensor(-float("inf")))
    x[at:at + ties] = tied
    nb = -(-V // 2048)                      # the launch's slices: ceil(V / (256 threads * 8 entries)) of ceil(V / nb) entries
    chunk = -(-V // nb)
    above, equal = int((x > tied).sum()), int((x == tied).sum())
    assert above < k <= above + equal and 1 <= k <= 64, (above, equal, k)          # the k-th largest value IS the tied one, on the fast route
    assert at + ties <= chunk and int((x[:chunk] == tied).sum()) > 64                # more than 64 of them in slice 0 alone
    assert int((x[:chunk] > tied).sum()) < 64                                        # ... so the slice's 64th value is the tied one and ties are dropped
    return x


def _params(rows, device):
    from videoglamm_amd import ops
    return torch.stack([ops.sampling_params(T, k, p, seed, device) for T, k, p, seed in rows])


def _single(x, params, step, u, fast):
    """row by row on vg_sample_partial: (acc [B], tok [B])"""
    from videoglamm_amd import ops
    B = x.shape[0]
    acc = torch.zeros(B, dtype=torch.int64, device=x.device)
    tok = torch.full((B,), -1, dtype=torch.int64, device=x.device)
    ws = ops.sample_workspace(x.device) if fast else None
    for b in range(B):
        ops.sample_partial(x[b], params[b], step[b:b + 1], acc=acc[b:b + 1], tok=tok[b:b + 1], u_override=None if u is None else u[b:b + 1], fast_ws=ws)
    return acc, tok


def _rows(x, params, step, u, ws):
    from videoglamm_amd import ops
    B = x.shape[0]
    acc = torch.zeros(B, dtype=torch.int64, device=x.device)
    tok = torch.full((B,), -1, dtype=torch.int64, device=x.device)
    ops.sample_partial_rows(x, params, step, acc=acc, tok=tok, u_override=u, fast_ws=ws)
    return acc, tok


def _mixed(B, route, seed):
    """B parameter rows (T, k, p, seed) that differ in every field, all on one route"""
    g = torch.Generator().manual_seed(seed)
    Ts = (0.3, 0.6, 1.0, 1.7)
    ps = (0.1, 0.9, 1.0, 0.5)
    fast_k = (1, 5, 50, 64, 20, 33, 2, 63)
    out = []
    for b in range(B):
        k = fast_k[(b + seed) % len(fast_k)] if route == "fast" else (0, 200)[(b + seed) % 2]
        out.append((Ts[(b + seed) % 4], k, ps[(b * 3 + seed) % 4], int(torch.randint(0, 2 ** 62, (1,), generator=g))))
    return out


def _check(x, params, step, u, fast):
    from videoglamm_amd import ops
    ws = ops.sample_workspace_rows(x.shape[0], x.device) if fast else None
    want = _single(x, params, step, u, fast)
    got = _rows(x, params, step, u, ws)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())
    assert torch.equal(0xFFFFFFFF - (got[0] & 0xFFFFFFFF), got[1])        # the key's low word is ~index
    if fast:
        assert int(ws[:, -64].abs().sum()) == 0                           # every row's ticket reset itself
    return got


@pytest.mark.parametrize("route", ["fast", "general"])
@pytest.mark.parametrize("B", [2, 5, 16])
@pytest.mark.parametrize("V", [8192, 32064, 128256])
def test_rows_equal_single_row_launches(cuda, V, B, route):
    fast = route == "fast"
    x = _logits(B, V, 11 * B + V % 7).to(cuda)
    params = _params(_mixed(B, route, B + V % 5), cuda)
    step = torch.arange(3, 3 + 7 * B, 7, dtype=torch.int32, device=cuda)
    a = _check(x, params, step, None, fast)
    u = torch.rand(B, generator=torch.Generator().manual_seed(V + B)).to(cuda)
    u[0] = 0.0
    _check(x, params, step, u, fast)
    # another step word per row draws from another Philox counter: at least the flat rows (high T, wide p) move
    hot = _params([(40.0, 50 if fast else 0, 1.0, 77 + b) for b in range(B)], cuda)
    t0 = _check(x, hot, step, None, fast)[1]
    t1 = _check(x, hot, step + 1, None, fast)[1]
    assert not torch.equal(t0, t1)
    assert a[1].min() >= 0 and a[1].max() < V


@pytest.mark.parametrize("V", [8192, 32064])
def test_rows_with_a_row_stride(cuda, V):
    """logits rows that are a column slice of a wider tensor (ldx > n)"""
    from videoglamm_amd import ops
    B = 5
    wide = _logits(B, V, 5, pad=64).to(cuda)
    x = wide[:, :V]
    assert not x.is_contiguous()
    params = _params(_mixed(B, "fast", 1), cuda)
    step = torch.arange(B, dtype=torch.int32, device=cuda)
    want = _single(x.contiguous(), params, step, None, True)
    got = _rows(x, params, step, None, ops.sample_workspace_rows(B, cuda))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    want = _single(x.contiguous(), params, step, None, False)
    got = _rows(x, params, step, None, None)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("k", [40, 50, 64])
@pytest.mark.parametrize("V", [8192, 128256])
def test_one_row_overflows_on_ties(cuda, V, k):
    """exactly one row of a fast-route batch has 90 entries of ONE slice tied at the global k-th value (_tie_block checks that on the host): its
    slice keeps 64 and flags the rest, and the row's last workgroup runs the general route for that row — on the row's own logits, parameter
    block, step word and outputs — inside the launch; the other rows stay on the fast route.  The rows differ in T, p, seed and step, so a
    fallback that picked another row's logits or parameters draws another token."""
    B, bad = 5, 3
    x = _logits(B, V, 21)
    _tie_block(x[bad], 90, k)
    for b in range(B):
        if b != bad:                        # the other rows do not overflow: no value of theirs is repeated more than 64 times
            assert int(torch.unique(x[b], return_counts=True)[1].max()) <= 64
    x = x.to(cuda)
    params = _params([((1.0, 1.7, 0.6, 1.3, 0.8)[b], k, (1.0, 0.9, 1.0, 1.0, 0.5)[b], 100 + b) for b in range(B)], cuda)
    step = torch.arange(2, 2 + B, dtype=torch.int32, device=cuda)
    # u near the top of the CDF: the last tied entries by index are the ones a slice had to drop
    seen = set()
    for uu in (0.0, 0.37, 0.995, 0.9995):
        u = torch.full((B,), uu, dtype=torch.float32, device=cuda)
        got = _check(x, params, step, u, True)
        gen = _single(x, params, step, u, False)
        assert torch.equal(got[0], gen[0])          # ... and both equal the general route
        seen.add(int(got[1][bad]))
    assert any(1000 + 64 <= t < 1000 + 90 for t in seen), seen      # the draws near u = 1 land in the tail of the tied run (ties go by ascending index)
    _check(x, params, step, None, True)                              # ... and with each row's own Philox uniform


def test_consecutive_launches_reuse_the_workspaces(cuda):
    """two launches on the same B workspaces, the second with other rows: the tickets reset per row and no candidate of launch 1 survives"""
    from videoglamm_amd import ops
    B, V = 5, 32064
    ws = ops.sample_workspace_rows(B, cuda)
    for rnd in range(3):
        x = _logits(B, V, 40 + rnd).to(cuda)
        if rnd == 1:
            x[2] = _tie_block(x[2].cpu(), 90, 50).to(cuda)  # an overflow row in between leaves its workspace reusable too
        params = _params(_mixed(B, "fast", rnd) if rnd != 1 else [(1.0, 50, 1.0, b) for b in range(B)], cuda)
        step = torch.full((B,), rnd, dtype=torch.int32, device=cuda)
        want = _single(x, params, step, None, True)
        got = _rows(x, params, step, None, ws)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), rnd
        assert int(ws[:, -64].abs().sum()) == 0


@pytest.mark.parametrize("V", [8192, 32064])
def test_k_outside_the_fast_range_on_the_fast_entry(cuda, V):
    """rows whose k is outside 1..64 (0, 65, 200, > V) among fast rows on the fast entry: those rows fall back inside the launch"""
    ks = [0, 50, 65, 200, V + 7, 64, 1]
    B = len(ks)
    x = _logits(B, V, 9).to(cuda)
    params = _params([((0.6, 1.0, 1.7)[b % 3], k, (0.9, 1.0)[b % 2], 500 + b) for b, k in enumerate(ks)], cuda)
    step = torch.arange(B, dtype=torch.int32, device=cuda)
    got = _check(x, params, step, None, True)
    gen = _single(x, params, step, None, False)
    assert torch.equal(got[0], gen[0]) and torch.equal(got[1], gen[1])


def test_argument_checks(cuda):
    from videoglamm_amd import _lib, ops
    x = _logits(2, 8192, 1).to(cuda)
    params = _params(_mixed(2, "fast", 0), cuda)
    step = torch.zeros(2, dtype=torch.int32, device=cuda)
    with pytest.raises(AssertionError):
        ops.sample_partial_rows(x, params, step)                                     # neither acc nor tok
    with pytest.raises(AssertionError):
        ops.sample_partial_rows(x, params, step, tok=torch.zeros(2, dtype=torch.int64, device=cuda), fast_ws=ops.sample_workspace(cuda))   # one workspace for two rows
    big = torch.zeros(1, 131073, device=cuda)
    with pytest.raises(_lib.VGKernelError):
        ops.sample_partial_rows(big, params[:1], step[:1], tok=torch.zeros(1, dtype=torch.int64, device=cuda), fast_ws=ops.sample_workspace_rows(1, cuda))
