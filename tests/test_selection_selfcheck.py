"""The case lists of tests/_select_ref.py cannot be passed by a wrong kernel: a numpy model of vg_argmax's two stages and one of
vg_multimask_select, each with a `mutant` switch, are run over the very cases the GPU test runs.  The unmutated models pass every case; every
mutant fails at least one NAMED case — except argmax's `stride_256`, which no input can tell from the kernel (see
test_stride_256_is_output_equivalent) and is kept, asserted equivalent, so that the list stays whole.

Counts (printed by test_counts): 15 row lengths, 376 argmax cases per dtype (x 2 dtypes), 9 argmax mutants (8 killed, 1 proven
output-equivalent); 5 mask sizes x 16 selection cases x 2 modes, 8 selection mutants (8 killed)."""
import numpy as np
import pytest
import torch

import _select_ref as R

ARGMAX_MUTANTS = ("tie_highest_index", "tie_lowest_workgroup", "no_sign_handling", "bit_order_zeros", "drop_last_stripe", "stride_256",
                  "nb_unclamped", "flush_denormals", "wrong_ldx")
SELECT_MUTANTS = ("best_ge", "best_from_0", "stab_gt", "delta_ge", "empty_gives_0", "lose_tail", "count_over_best", "stable_returns_best_iou")


# ---- a numpy model of argmax_stage1 + argmax_stage2 ----------------------------------------------------------------------------------------
def argmax_model(x, mutant=None):
    """x fp32 [rows, n] -> int64 [rows]: every thread's entries keyed (ordered value bits, ~index), the largest key of the row decoded.
    The geometry enters through which entries are read at all and, for the workgroup tie mutant, through who read them."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, n = x.shape
    flat = x.reshape(-1)
    nb = R.nb_of(n)
    i = np.arange(n, dtype=np.int64)
    # which entries some thread reads: thread (wg, t) walks i = wg*256 + t + trip*stride while i < bound
    stride, bound = nb * R.WG, n
    if mutant == "nb_unclamped":
        stride = -(-n // R.PER_WG) * R.WG                 # the kernel argument unclamped, the grid still 64 workgroups
    if mutant == "stride_256":
        stride = R.WG
    if mutant == "drop_last_stripe":
        bound = n - n % R.WG
    read = ((i % stride) < nb * R.WG) & (i < bound)
    out = np.empty(rows, np.int64)
    for r in range(rows):
        ldx = n + 1 if mutant == "wrong_ldx" else n
        v = flat[np.minimum(r * ldx + i, flat.size - 1)]  # (the model stays inside the buffer; the kernel would not)
        if mutant != "bit_order_zeros":
            v = v + np.float32(0.0)                       # -0 counts as +0
        if mutant == "flush_denormals":
            v = np.where(np.abs(v) < R.FLT_MIN, np.float32(0.0), v)
        u = v.view(np.uint32).astype(np.uint64)
        neg = (u & np.uint64(0x80000000)) != 0
        if mutant == "no_sign_handling":
            neg = np.zeros(n, bool)
        key = np.where(neg, ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000))
        if mutant == "tie_highest_index":
            low = i.astype(np.uint64)
        elif mutant == "tie_lowest_workgroup":
            wg = (i % (nb * R.WG)) // R.WG
            low = np.uint64(0xffffffff) - ((wg.astype(np.uint64) << np.uint64(20)) | i.astype(np.uint64))
        else:
            low = np.uint64(0xffffffff) - i.astype(np.uint64)
        k = np.where(read, (key << np.uint64(32)) | low, np.uint64(0))
        best = int(k.max()) & 0xffffffff                  # acc starts at zero: a row nobody reads decodes to 0xffffffff
        if mutant == "tie_highest_index":
            out[r] = best
        elif mutant == "tie_lowest_workgroup":
            out[r] = (0xffffffff - best) & 0xfffff
        else:
            out[r] = 0xffffffff - best
    return out


def _argmax_failures(mutant, bf16):
    failed = []
    for n in R.NS:
        for name, row, want in R.cases(n, bf16):
            if int(argmax_model(row[None], mutant)[0]) != want:
                failed.append(f"{n}-{name}")
        if mutant == "wrong_ldx" or mutant is None:
            for rows in (3, 16):
                names, x, want = R.pack(n, rows, bf16, start=rows)
                got = argmax_model(x, mutant)
                failed += [f"{n}-rows{rows}-{nm}" for nm, g, w in zip(names, got, want) if g != w]
    return failed


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_reference_and_cases_agree(bf16):
    """every case's stated index is first_max of its row and torch.argmax's on the CPU; the bf16 rows survive the cast unchanged"""
    total = 0
    for n in R.NS:
        names = R.case_names(n)
        assert len(set(names)) == len(names)
        for name, row, want in R.cases(n, bf16):
            assert row.dtype == np.float32 and row.shape == (n,) and not np.isnan(row).any()
            t = torch.from_numpy(row)
            assert R.first_max(row) == want == int(torch.argmax(t)), (n, name)
            if bf16:
                tb = t.to(torch.bfloat16)
                assert np.array_equal(tb.float().numpy().view(np.uint32), row.view(np.uint32)), (n, name)
                assert int(torch.argmax(tb)) == want, (n, name)
            total += 1
    assert total == 376, total


def test_geometry_model():
    for n in R.NS:
        nb = R.nb_of(n)
        assert 1 <= nb <= 64
        seen = np.zeros(n, int)
        for i in (0, 1, 255, 256, n // 2, n - 1):
            if 0 <= i < n:
                wg, wave, lane, trip = R.owner(i, n)
                assert R.index_of(wg, wave * 64 + lane, trip, n) == i and wg < nb
        i = np.arange(n)
        seen[i] += 1                                       # every entry has exactly one owner: (i % (nb*256)) // 256 < nb always
        assert ((i % (nb * 256)) // 256 < nb).all() and (seen == 1).all()
    assert R.nb_of(131072) == 64 == R.nb_of(131073) and R.nb_of(2049) == 2 and R.nb_of(2048) == 1
    assert R.owner(300, 32064)[0] == 1 and R.owner(256 * 16 + 5, 32064) == (0, 0, 5, 1)
    for n in (2049, 32064, 128256, 200003):                # the pairings the issue names exist where the row is long enough
        have = {nm for nm, _, _ in R.tie_pairs(n)}
        assert {"tie_same_wave", "tie_two_waves", "tie_two_trips", "tie_two_workgroups", "tie_hi_in_lower_workgroup"} <= have, (n, have)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_unmutated_argmax_model_passes_every_case(bf16):
    assert _argmax_failures(None, bf16) == []


@pytest.mark.parametrize("mutant", [m for m in ARGMAX_MUTANTS if m != "stride_256"])
def test_every_argmax_mutant_fails_a_named_case(mutant):
    for bf16 in (False, True):
        failed = _argmax_failures(mutant, bf16)
        assert failed, (mutant, bf16)
        print(mutant, "bf16" if bf16 else "fp32", len(failed), "cases, e.g.", failed[:3])


def test_signed_zero_mutant_is_todays_regression():
    """the bit-order mutant is the kernel before `v + 0`: it fails the -0-before-+0 cases and nothing else"""
    for bf16 in (False, True):
        failed = _argmax_failures("bit_order_zeros", bf16)
        assert failed and all(R.is_signed_zero_case(f.split("-", 1)[1]) for f in failed), failed
        assert len(failed) == sum(R.is_signed_zero_case(nm) for n in R.NS for nm in R.case_names(n))


def test_stride_256_is_output_equivalent():
    """a stride of 256 where nb*256 belongs makes workgroup wg read EVERY entry from wg*256 on: workgroup 0 reads the whole row and the others
    re-read parts of it.  The maximum key over a multiset that covers the row is the row's maximum key, so the output cannot differ on any
    input — only the time can.  No case can kill this mutant; it stays in the list, asserted equivalent."""
    for n in R.NS:
        i = np.arange(n)
        assert ((i % 256) < R.nb_of(n) * 256).all()        # the model's read set: everything
    assert _argmax_failures("stride_256", False) == []


# ---- a numpy model of multimask_select_kernel / multimask_best_kernel -------------------------------------------------------------------
def select_model(masks, ious, mode, mutant=None):
    """masks fp32 [N, 4, HW], ious fp32 [N, 4] -> (mask token [N], iou [N] fp32, token row [N]) as the kernel picks them"""
    N, _, HW = masks.shape
    sel_out, iou_out, tok_out = np.empty(N, int), np.empty(N, np.float32), np.empty(N, int)
    for n in range(N):
        io = ious[n]
        best = 0 if mutant == "best_from_0" else 1
        for k in range(best + 1, 4):
            if (io[k] >= io[best]) if mutant == "best_ge" else (io[k] > io[best]):
                best = k
        sel = best
        stable = False
        if mode == 0:
            m = masks[n, best if mutant == "count_over_best" else 0]
            if mutant == "lose_tail":
                m = m[: HW - HW % 4]
            if mutant == "delta_ge":
                ai, au = np.float32((m >= R.DELTA).sum()), np.float32((m >= -R.DELTA).sum())
            else:
                ai, au = np.float32((m > R.DELTA).sum()), np.float32((m > -R.DELTA).sum())
            stab = ai / au if au > 0 else np.float32(0.0 if mutant == "empty_gives_0" else 1.0)
            stable = stab > R.THRESH if mutant == "stab_gt" else stab >= R.THRESH
            sel = 0 if stable else best
        sel_out[n] = sel
        iou_out[n] = io[best] if (stable and mutant == "stable_returns_best_iou") else io[sel]
        tok_out[n] = 0 if mode == 0 else sel
    return sel_out, iou_out, tok_out


def _select_failures(mutant):
    failed = []
    for HW in R.HWS:
        names, masks, ious, best, stable = R.selection_cases(HW)
        tokens = torch.arange(len(names) * 4, dtype=torch.float32).view(-1, 4, 1)          # a token row that names itself
        for mode in (0, 1):
            rm, ri, rt, rx = R.multimask_select(torch.from_numpy(masks).view(len(names), 4, 1, HW), torch.from_numpy(ious), tokens, mode,
                                                delta=float(R.DELTA), thresh=float(R.THRESH))
            sel, iou, tok = select_model(masks, ious, mode, mutant)
            for c, name in enumerate(names):
                ok = sel[c] == int(rx[c]) and iou[c] == float(ri[c]) and c * 4 + tok[c] == int(rt[c, 0])
                if not ok:
                    failed.append(f"{HW}-mode{mode}-{name}")
    return failed


def test_selection_cases_say_what_they_claim():
    assert np.float32(49) / np.float32(50) == np.float32(0.98) == R.THRESH
    for HW in R.HWS:
        k = HW // 50
        assert np.float32(49 * k) / np.float32(50 * k) == R.THRESH and np.float32(49 * k - 1) / np.float32(50 * k) < R.THRESH
        names, masks, ious, best, stable = R.selection_cases(HW)
        assert len(names) == len(set(names)) == len(R.iou_rows()) == 16
        N = len(names)
        assert (ious[:, 0:1] > ious[:, 1:]).all()                       # token 0's IoU is the largest of the four: never the pick in mode 1
        m4 = torch.from_numpy(masks).view(N, 4, 1, HW)
        for mode in (0, 1):
            rm, ri, rt, rx = R.multimask_select(m4, torch.from_numpy(ious), torch.zeros(N, 4, 2), mode, delta=float(R.DELTA), thresh=float(R.THRESH))
            want = np.where(stable, 0, best) if mode == 0 else best
            assert rx.tolist() == want.tolist(), (HW, mode)
            assert torch.equal(rm.view(N, HW), torch.from_numpy(masks[np.arange(N), want]))
        assert torch.equal(torch.argmax(torch.from_numpy(ious[:, 1:]), dim=-1) + 1, torch.from_numpy(best))
        # the pads: pixels exactly on +delta and on -delta exist in token 0's mask wherever their group is not empty, and the reference
        # counts neither as above its bound
        for c, name in enumerate(names):
            m = masks[c, 0]
            a, u = int((m > R.DELTA).sum()), int((m > -R.DELTA).sum())
            if u > a:
                assert (m == R.DELTA).any(), (HW, name)
            if HW > u:
                assert (m == -R.DELTA).any(), (HW, name)
            t = torch.from_numpy(m)
            assert int((t > 0.05).sum()) == a and int((t > -0.05).sum()) == u       # torch compares in fp32, as the kernel does
        for c in range(N):                                              # the four masks of a case differ: a wrong pick shows in the output mask
            assert len({masks[c, t].tobytes() for t in range(4)}) == 4


def test_unmutated_selection_model_passes_every_case():
    assert _select_failures(None) == []


@pytest.mark.parametrize("mutant", SELECT_MUTANTS)
def test_every_selection_mutant_fails_a_named_case(mutant):
    failed = _select_failures(mutant)
    assert failed, mutant
    print(mutant, len(failed), "cases, e.g.", failed[:3])


def test_specials():
    x = torch.from_numpy(R.SPECIALS)
    assert (x > 0).tolist() == R.SPECIALS_POSITIVE.tolist() and len(R.SPECIALS) == 11
    y, pos = R.specials_in_noise(2 ** 20 + 3, 0)
    assert len(set(pos.tolist())) == len(pos) == 55 and np.array_equal(y[pos].view(np.uint32), np.tile(R.SPECIALS, 5).view(np.uint32))


def test_counts(capsys):
    per = {n: len(R.case_names(n)) for n in R.NS}
    with capsys.disabled():
        print(f"\nargmax: {len(R.NS)} row lengths, {sum(per.values())} cases per dtype {per}, {len(ARGMAX_MUTANTS)} mutants; "
              f"selection: {len(R.HWS)} mask sizes x {len(R.iou_rows())} cases x 2 modes, {len(SELECT_MUTANTS)} mutants")
    assert len(ARGMAX_MUTANTS) == 9 and len(SELECT_MUTANTS) == 8
