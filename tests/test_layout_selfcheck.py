"""The power of tests/test_layout_spatial_gpu.py and tests/test_decoder_fused_gpu.py, proven on the CPU (no GPU, not marked gpu).

On the designs of tests/_layout_ref.py:
  * the CPU fp32 statement of every design (tests/_cpu_ops.py where it has one, the fp32 chains of _layout_ref otherwise) passes its own check;
  * each wrong kernel fails every case of every class it applies to.  The grid-stride ones (second-pass items not written, second pass reading the first
    pass's inputs, last work item dropped) apply to every kernel with a capped grid: the first two to the cases past one pass, the third to all.  The
    others apply where the kernel has that stage: a border tap taken from the clamped pixel (im2col with padding, dwconv, conv3s2_ln_gelu), the strip
    tail written past W (dwconv strip, W % 4 != 0), the Kpad tail (im2col, Kpad > Kreal), a window's padding token (ragged H or W), >= 0 for > 0
    (bilinear_mask), x1 not clamped (bilinear and bilinear_mask when upscaling: at scale 1/2 the last column's x0 is Wi - 2).
  * two-way: every wrong kernel but the missing rounding of the probabilities fails every selector case it applies to (the instance maps where
    1 < Nx < N, the five that act on scores or probabilities where nt > 1: with one token every probability is 1); the missing rounding fails the random-data cases (in the selector
    design it moves y by less than y's own bf16 rounding).
  * upscale: the index mutants fail the saturating and the random design, eps x 10 the quiet design, tanh GELU the quiet and the random design (beyond
    +-8 the two GELUs agree: not the saturating one), 63 channels and the missing rounding all three.
The largest cases of the GPU tests (tens of millions of elements) are not rebuilt here: every kernel's second pass is represented by its cheapest
past-one-pass case, and the pointwise tail / head design by stand-ins at the GPU tests' sizes.
"""
import pytest
import torch

import _layout_ref as L
import _rowwise_ref as R

torch.set_grad_enabled(False)
BF, F32 = L.BF, L.F32


def _small():
    return (L.permute5_cases(False) + L.im2col_cases(False) + L.dwconv_cases(False) + L.shuffle_cases(False) + L.pool2_cases(False) + L.window_cases(False)
            + L.bilinear_cases(False) + L.heads_cases(False))


def _past():
    """the cheapest past-one-pass case of every capped launcher"""
    d, H, W = (2, 420, 420, 3, 1), 420, 420
    return ([L.permute5_case("permute5 past one pass", d, (3 * H * W, W, 1, H * W, 0), 2 * 3 * H * W, BF, 2),
             L.im2col_case("im2col past one pass", 1, 324, 324, 3, 7, 4, 3, 160, BF, 3),
             L.dwconv_case("dwconv strip past one pass", 2731, 3, 5, 512, 7, BF, 5, sel_big=(2, 3)),
             L.dwconv_case("dwconv scalar past one pass", 1, 297, 295, 12, 3, BF, 6),
             L.pixel_shuffle2_case("pixel_shuffle2 past one pass", 1, 181, 182, 8, BF, seed=3),
             L.upsample2_add_case("upsample2_add past one pass", 1, 181, 182, 8, F32, 4),
             L.pool2_case("pool2 scalar past one pass", 1, 918, 914, 5, 5, 0, BF, False, 7),
             L.heads_case(33, 9, 16, BF, False, 20), L.heads_case(461, 9, 16, BF, True, 21)]
            + list(L.window_cases_one("window scalar past one pass", 1, 297, 297, 12, 7, BF, 30))
            + list(L.bilinear_cases_one("bilinear past one pass", 1, 511, 515, 1022, 1030, 8)[:1]))


@pytest.fixture(scope="module")
def small():
    return _small()


@pytest.fixture(scope="module")
def past():
    cs = _past()
    for c in cs:
        assert c.past() and (L.past_one_pass(c.n_items, c.cap) or c.route == "heads_bd_kernel"), (c.name, c.n_items)
    return cs


def test_statements_pass_exact(small, past):
    for c in small + past:
        assert L.passes(c, c.stmt.reshape(c.want.shape)), c.name


def _mutants_of(c):
    return list(L.GRID_MUTANTS) + list(c.aux)


def test_wrong_kernels_fail_exact(small, past):
    seen = {}
    for c in small + past:
        for m in _mutants_of(c):
            o = L.mutate(c, m)
            if o is None:
                continue
            assert not L.passes(c, o), (c.name, m)
            seen.setdefault(m, set()).add(c.route)
    # every wrong kernel met every route that has its stage
    capped = {c.route for c in small + past if c.cap < 1 << 40}
    assert seen[L.GRID_MUTANTS[2]] >= capped
    for m in L.GRID_MUTANTS[:2]:
        assert seen[m] == {c.route for c in past}, (m, seen[m])
    assert {"im2col_kernel", "dwconv_kernel", "dwconv_strip_kernel<7>"} <= seen["a border tap taken from the clamped pixel instead of skipped"]
    assert seen["strip tail pixel written past W"] == {"dwconv_strip_kernel<7>"} and seen["Kpad tail not zeroed"] == {"im2col_kernel"}
    assert seen["window padding token not zeroed"] == {"window_part_kernel scalar", "window_part_kernel chunk"}
    assert seen["`>= 0` for `> 0`"] == {"bilinear_mask_rows_kernel", "bilinear_mask_kernel"}
    assert seen["bilinear x1 not clamped at the last column"] == {"bilinear_kernel", "bilinear_mask_rows_kernel", "bilinear_mask_kernel"}


def test_unpartition_gives_the_image_back(small):
    parts = [c for c in small if c.name.endswith(" partition")]
    assert parts
    for c in parts:
        x = c.call["x"]
        u = [k for k in small if k.name == c.name.replace(" partition", " unpartition")][0]
        assert torch.equal(u.want, x) and bool((c.want[u.call["win"] == 2.0 ** 10] == 0).all())


def _conv_cases():
    return L.conv3s2_cases(False) + [L.conv3s2_case("conv3s2 1->4 past one pass", 4099, 30, 34, 1, 4, BF, 9, sel_big=(4, 4))]


def test_conv3s2_statement_passes_and_wrong_kernels_fail():
    for ex, case in _conv_cases():
        r = case.evaluate(case.cpu32.to(case.out_dtype))
        assert r["ok"], (ex.name, r)
        case.precondition()
        n = 0
        for m in _mutants_of(ex):
            o = L.mutate(ex, m)
            if o is None:
                continue
            n += 1
            assert not case.evaluate(o)["ok"], (ex.name, m)
        assert n >= (4 if ex.past() else 2), ex.name


@pytest.mark.parametrize("unit", [1, 8])
def test_tail_equals_head_design(unit):
    """the pointwise tail / head design with an honest stand-in (an erf GELU in fp32 on the repeated input) and the three wrong grid-stride loops"""
    n = L.pointwise_n(unit)
    src, tail = L.repeat_tail(n, unit)
    base = torch.randn(n, generator=torch.Generator().manual_seed(unit))
    out = torch.nn.functional.gelu(base[src]).to(BF)
    assert int(tail.sum()) == 1337 * unit and L.tail_equals_head(out, n, unit)
    for m in L.GRID_MUTANTS:
        assert not L.tail_equals_head(L.tail_mutant(out, n, unit, m), n, unit), m


# ------------------------------------------------------------------ two-way
SELECTOR = [(3, 3, 40, 7, 8), (4, 2, 296, 1, 8), (3, 1, 40, 8, 8), (4, 2, 40, 9, 16), (3, 1, 296, 16, 16), (3, 3, 40, 1, 16), (4, 2, 40, 8, 16)]      # N, Nx, P, nt, TP


def _twoway_applies(m, N, Nx, nt):
    if m == L.TWOWAY_MUTANTS[8]:
        return False
    if m in (L.TWOWAY_MUTANTS[5], L.TWOWAY_MUTANTS[6]):
        return 1 < Nx < N
    if m in L.TWOWAY_MUTANTS[:5]:          # (one token: every probability is 1 whatever the scores are)
        return nt > 1
    return True


def _selector_verdict(d, case, xo, xpo):
    ok = case.evaluate(xo.reshape(-1, 256))["ok"]
    return ok and torch.equal(xpo, (xo.float() + d["pe"].float()).to(BF))


@pytest.mark.parametrize("N,Nx,P,nt,TP", SELECTOR)
def test_twoway_selector(N, Nx, P, nt, TP):
    d = L.twoway_selector(N, Nx, P, nt, TP, seed=nt)
    case = L.twoway_selector_case(d)
    case.precondition()
    xo, xpo = L.twoway_model(d)
    r = case.evaluate(xo.reshape(-1, 256))
    print(R.line(case, r))
    assert r["ok"] and _selector_verdict(d, case, xo, xpo)
    for m in L.TWOWAY_MUTANTS:
        if _twoway_applies(m, N, Nx, nt):
            assert not _selector_verdict(d, case, *L.twoway_model(d, m)), m
    assert not _selector_verdict(d, case, xo, (xo.float() + d["pe"].float() * 1.01).to(BF))


@pytest.mark.parametrize("TP,nt", [(8, 7), (16, 9)])
def test_twoway_random(TP, nt):
    d = L.twoway_random(3, 3, 296, nt, TP, seed=TP)
    chk = L.twoway_random_check(d)
    chk.precondition()
    r = chk.evaluate(L.twoway_model(d)[0])
    print(chk.name, r)
    assert r["ok"]
    for m in (L.TWOWAY_MUTANTS[8], L.TWOWAY_MUTANTS[0], L.TWOWAY_MUTANTS[1], L.TWOWAY_MUTANTS[3]):
        rm = chk.evaluate(L.twoway_model(d, m)[0])
        print(m, rm)
        assert not rm["ok"], m


# ------------------------------------------------------------------ mask upscale
UP = L.UPSCALE_MUTANTS
UP_APPLIES = {"random": (UP[0], UP[1], UP[2], UP[3], UP[5], UP[6]), "saturating": (UP[0], UP[1], UP[2], UP[3], UP[6]), "quiet": (UP[3], UP[4], UP[5], UP[6])}


@pytest.mark.parametrize("design", ["random", "saturating", "quiet"])
def test_upscale_designs(design):
    d = L.upscale_random(4, 2, 8, seed=3, design=design)
    chk = L.upscale_check(d, design)
    chk.precondition()
    r = chk.evaluate(L.upscale_chain(d, F32))
    print(design, r)
    assert r["ok"]
    if design == "saturating":          # every GELU argument beyond +-8
        a1, a2 = L.upscale_arguments(d)
        assert float(a1.abs().min()) > 8 and float(a2.abs().min()) > 8
    for m in UP_APPLIES[design]:
        rm = chk.evaluate(L.upscale_chain(d, F32, m))
        print(m, rm)
        assert not rm["ok"], (design, m)
