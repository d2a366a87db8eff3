"""References and inputs for the kernels that make discrete decisions (tests/test_selection_gpu.py, tests/test_selection_selfcheck.py): the
argmax family (vg_argmax, vg_argmax_partial, vg_decode_step_end(_rows)), SAM2's mask selection (vg_multimask_select) and the strict `> 0`
deciders.  Pure numpy / torch-CPU.

Argmax: the reference is first_max — the lowest index holding the row maximum, compared in float64 (the upcast is exact, so -0 == +0); rows
are NaN-free, as include/vg_kernels.h states.  owner() restates the kernel's geometry (argmax_stage1: nb = min(64, ceil(n / 2048)) workgroups
of 256 threads, thread t of workgroup wg reads i = wg*256 + t + trip*nb*256), so that the case builders can put a maximum or a tie at a chosen
workgroup, wave, lane and trip.  Every planted value is bf16-representable where the case is built for bf16: the reference sees the stored
values.

Mask selection: the reference is tests/_cpu_ops.multimask_select (SAM2's _dynamic_multimask_via_stability and best-IoU rule); the builders
here make token-0 masks with prescribed pixel counts above +delta and above -delta, padded with pixels exactly on +-delta, and the IoU rows
of the best-of-3 rule."""
import functools
import itertools

import numpy as np
import torch

from _cpu_ops import multimask_select  # noqa: F401  (the mask-selection reference: imported, not restated)

# ---- argmax ------------------------------------------------------------------------------------------------------------------------------
NS = (1, 63, 64, 65, 255, 256, 257, 2048, 2049, 4097, 32064, 128256, 131072, 131073, 200003)
WG = 256           # threads of a workgroup
PER_WG = 2048      # entries a workgroup is sized for
MAX_WG = 64

DENORM32 = np.float32(np.uint32(1).view(np.float32))                   # the smallest positive fp32 denormal
DENORM16 = np.float32(np.uint32(0x00010000).view(np.float32))          # the smallest positive bf16 denormal (a denormal in fp32 too)


def nb_of(n):
    return min(MAX_WG, -(-n // PER_WG))


def owner(i, n):
    """(workgroup, wave, lane, trip) of the thread that reads entry i of a row of n"""
    nb = nb_of(n)
    trip, r = divmod(i, nb * WG)
    wg, t = divmod(r, WG)
    return wg, t >> 6, t & 63, trip


def index_of(wg, t, trip, n):
    """the entry thread t of workgroup wg reads on its trip-th trip (it may lie past the row's end)"""
    return wg * WG + t + trip * nb_of(n) * WG


def first_max(x):
    x = np.asarray(x).astype(np.float64)
    return int(np.flatnonzero(x == x.max())[0])


def to_bf16_values(x):
    """x rounded to bf16, held in fp32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def filler(n, seed, bf16):
    x = np.random.default_rng(seed).uniform(-4.0, 4.0, n).astype(np.float32)
    x[x >= 4.0] = 3.5                      # (the cast of a double just under 4 can round up to it)
    return to_bf16_values(x) if bf16 else x


def negative_filler(n, seed, bf16):
    """random values in (-4.5, -0.5]"""
    x = -np.abs(filler(n, seed, False)) - np.float32(0.5)
    return to_bf16_values(x) if bf16 else x


def _last_wg_span(n):
    """first and last entry the last workgroup reads"""
    nb = nb_of(n)
    first = (nb - 1) * WG
    if first >= n:                         # (a row shorter than its last workgroup's first entry: that workgroup reads nothing)
        return None
    own = [i for i in range(max(first, n - nb * WG - WG), n) if owner(i, n)[0] == nb - 1]
    return first, (own[-1] if own else first + min(WG, n - first) - 1)


def tie_pairs(n):
    """(name, lo, hi): two entries that hold the same maximum, by who reads them"""
    nb = nb_of(n)
    pairs = [("tie_same_wave", index_of(0, 2, 0, n), index_of(0, 40, 0, n)),
             ("tie_two_waves", index_of(0, 10, 0, n), index_of(0, 200, 0, n)),
             ("tie_two_trips", index_of(0, 7, 0, n), index_of(0, 7, 1, n)),
             ("tie_adjacent", n - 2, n - 1)]
    if nb >= 2:
        pairs += [("tie_two_workgroups", index_of(0, 10, 0, n), index_of(1, 10, 0, n)),
                  ("tie_first_last_workgroup", index_of(0, 3, 0, n), index_of(nb - 1, 3, 0, n)),
                  ("tie_hi_in_lower_workgroup", 300, WG * nb + 5)]       # slices interleave: 300 is workgroup 1's, 256*nb + 5 workgroup 0's second trip
    out = []
    for name, lo, hi in pairs:
        if 0 <= lo < hi < n:
            if name == "tie_hi_in_lower_workgroup":
                assert owner(hi, n)[0] < owner(lo, n)[0]
            out.append((name, lo, hi))
    return out


@functools.lru_cache(maxsize=None)
def case_specs(n):
    """[(name, build)]: build(bf16) -> (row fp32 [n] (bf16-representable values when bf16), expected index).  Names are stable: they are the
    test ids."""
    specs = []
    seed = [n * 1000]

    def add(name, fn):
        seed[0] += 1
        s = seed[0]
        specs.append((name, lambda bf16, fn=fn, s=s: fn(s, bf16)))

    def unique_at(i):
        def fn(s, bf16):
            x = filler(n, s, bf16)
            x[i] = 5.0
            return x, i
        return fn

    where = {0: "0", 1: "1", 255: "255", 256: "256", n - 2: "n-2", n - 1: "n-1"}
    nb = nb_of(n)
    where.setdefault(nb * WG - 1, "trip0_last")             # the last entry of everybody's first trip and the first of the second
    where.setdefault(nb * WG, "trip1_first")
    span = _last_wg_span(n)
    if span:
        where.setdefault(span[0], "lastwg_first")
        where.setdefault(span[1], "lastwg_last")
    for i, tag in sorted(where.items()):
        if 0 <= i < n:
            add("unique_at_" + tag, unique_at(i))

    def tie_at(lo, hi):
        def fn(s, bf16):
            x = filler(n, s, bf16)
            x[lo] = x[hi] = 6.0
            return x, lo
        return fn

    for name, lo, hi in tie_pairs(n):
        add(name, tie_at(lo, hi))

    add("all_equal", lambda s, bf16: (np.full(n, -1.25, np.float32), 0))
    add("all_neg_inf", lambda s, bf16: (np.full(n, -np.inf, np.float32), 0))

    def huge_negative(s, bf16):
        # bf16 bit patterns 0xff63 .. 0xff7f: -3.02e38 .. -3.39e38, every one <= -3e38; the largest, 0xff62 (-3.004e38), at n - 1
        bits = np.random.default_rng(s).integers(0xff63, 0xff80, n).astype(np.uint32) << 16
        x = bits.view(np.float32).copy()
        x[n - 1] = np.uint32(0xff62 << 16).view(np.float32)
        assert np.all(x <= -3e38) and np.all(np.isfinite(x))
        return x, n - 1

    add("all_below_-3e38_max_at_n-1", huge_negative)

    def one_inf(s, bf16):
        x = filler(n, s, bf16)
        i = (2 * n) // 3
        x[i] = np.inf
        return x, i

    add("one_pos_inf", one_inf)

    def denormal_max(s, bf16):
        x = negative_filler(n, s, bf16)
        x[::3] = 0.0
        x[1::7] = -0.0
        i = (3 * n) // 4
        x[i] = DENORM16 if bf16 else DENORM32
        return x, i

    add("denormal_max_over_zeros", denormal_max)

    def zeros(lo, hi, first):
        def fn(s, bf16):
            x = negative_filler(n, s, bf16)
            x[lo], x[hi] = (-0.0, 0.0) if first == "neg" else (0.0, -0.0)
            return x, lo
        return fn

    for name, lo, hi in tie_pairs(n):
        add("zeros_neg_first_" + name[4:], zeros(lo, hi, "neg"))
        add("zeros_pos_first_" + name[4:], zeros(lo, hi, "pos"))
    return specs


def case_names(n):
    return [name for name, _ in case_specs(n)]


def cases(n, bf16=False):
    """yields (name, row, expected_index)"""
    for name, build in case_specs(n):
        row, want = build(bf16)
        yield name, row, want


def build_case(n, name, bf16):
    return dict(case_specs(n))[name](bf16)


def is_signed_zero_case(name):
    return name.startswith("zeros_neg_first_")          # -0 at lo, +0 at hi: the bit order of the keys prefers hi


def pack(n, rows, bf16, start=0):
    """`rows` different cases of the same n as one [rows, n] array (cycling through the case list from `start`) -> (names, x, expected [rows])"""
    specs = case_specs(n)
    pick = [specs[(start + r) % len(specs)] for r in range(rows)]
    built = [b(bf16) for _, b in pick]
    return [nm for nm, _ in pick], np.stack([x for x, _ in built]), np.array([w for _, w in built], np.int64)


# ---- mask selection ----------------------------------------------------------------------------------------------------------------------
DELTA = np.float32(0.05)
THRESH = np.float32(0.98)
HWS = (50, 63, 400, 4100, 65536)


def stability_mask(HW, a, u, seed, last=None):
    """fp32 [HW]: exactly `a` pixels > delta, `u` pixels > -delta (the a included), the rest not; pixels exactly == delta sit among the u - a
    (above -delta, NOT above delta) and pixels exactly == -delta among the rest (NOT above -delta).  The groups are scattered over the whole
    mask.  last: "a" puts a pixel of the first group at HW - 1 and pixels of the rest at the other HW % 4 last positions."""
    assert 0 <= a <= u <= HW
    rng = np.random.default_rng(seed)
    hi = rng.uniform(0.06, 3.0, a).astype(np.float32)
    if a:
        hi[0] = np.nextafter(DELTA, np.float32(1))
    mid = rng.uniform(-0.04, 0.04, u - a).astype(np.float32)
    mid[: max(1, (u - a) // 3) if u > a else 0] = DELTA
    if u - a > 1:
        mid[-1] = np.nextafter(-DELTA, np.float32(0))
    lo = rng.uniform(-3.0, -0.06, HW - u).astype(np.float32)
    lo[: max(1, (HW - u) // 3) if HW > u else 0] = -DELTA
    vals = np.concatenate([hi, mid, lo])
    kind = np.concatenate([np.zeros(a, np.int8), np.ones(u - a, np.int8), np.full(HW - u, 2, np.int8)])
    perm = rng.permutation(HW)
    m, k = np.empty(HW, np.float32), np.empty(HW, np.int8)
    m[perm], k[perm] = vals, kind
    if last == "a":
        tail = list(range(HW - (HW % 4), HW - 1)) if HW % 4 else []
        want = [(HW - 1, 0)] + [(j, 2) for j in tail]
        for j, g in want:                                   # swap a pixel of group g into position j
            if k[j] != g:
                src = [q for q in np.flatnonzero(k == g) if q not in (HW - 1, *tail)]
                if not src:
                    continue
                q = src[0]
                m[j], m[q] = m[q], m[j]
                k[j], k[q] = k[q], k[j]
    assert int((m > DELTA).sum()) == a and int((m > -DELTA).sum()) == u
    return m


def iou_rows():
    """[(name, [iou1, iou2, iou3], expected token)]: the best-of-3 rule's rows.  Token 0's IoU, the largest of the four, is added by
    selection_cases."""
    rows = []
    for p in itertools.permutations((0.3, 0.5, 0.7)):
        rows.append(("order_" + "".join(str(int(v * 10)) for v in p), list(p), 1 + p.index(0.7)))
    for i, j in ((0, 1), (0, 2), (1, 2)):
        k = 3 - i - j
        v = [0.0, 0.0, 0.0]
        v[i] = v[j] = 0.6
        v[k] = 0.2
        rows.append((f"pair_{i + 1}{j + 1}_above", v, 1 + i))
        v = [0.0, 0.0, 0.0]
        v[i] = v[j] = 0.2
        v[k] = 0.6
        rows.append((f"pair_{i + 1}{j + 1}_below", v, 1 + k))
    rows.append(("all_tied", [0.4, 0.4, 0.4], 1))
    rows.append(("all_negative", [-0.5, -0.25, -0.75], 2))
    rows.append(("neg_zero_first", [-0.0, 0.0, -1.0], 1))
    rows.append(("pos_zero_first", [-1.0, 0.0, -0.0], 2))
    return rows


def stability_kinds(HW):
    """[(name, a, u, stable)] for token 0's mask; u is the largest multiple of 50 that fits: fp32(49k) / fp32(50k) == fp32(0.98)"""
    k = HW // 50
    return [("on_threshold", 49 * k, 50 * k, True), ("one_under", 49 * k - 1, 50 * k, False), ("empty", 0, 0, True),
            ("full", 50 * k, 50 * k, True), ("half", 25 * k, 50 * k, False)]


def selection_cases(HW, seed=0):
    """-> (names, masks fp32 [N, 4, HW], ious fp32 [N, 4], best [N], stable [N]): every IoU row, each with one of the stability kinds in
    turn (so every kind meets several rows).  Tokens 1..3 carry masks whose own stability is the OPPOSITE of token 0's, so a count taken over
    the wrong token decides the other way; token 0's IoU is the largest of the four."""
    rows, kinds = iou_rows(), stability_kinds(HW)
    names, masks, ious, best, stable = [], [], [], [], []
    for c, (rname, r, want) in enumerate(rows):
        kname, a, u, st = kinds[c % len(kinds)]
        m = np.empty((4, HW), np.float32)
        m[0] = stability_mask(HW, a, u, seed * 1000 + c, last="a" if kname == "on_threshold" else None)
        for t in range(1, 4):
            oa, ou = (0, HW) if st else (HW, HW)
            m[t] = stability_mask(HW, oa, ou, seed * 1000 + 100 * t + c)
        names.append(f"{rname}-{kname}")
        masks.append(m)
        ious.append([0.9] + r)
        best.append(want)
        stable.append(st)
    return names, np.stack(masks), np.array(ious, np.float32), np.array(best), np.array(stable)


# ---- the strict > 0 deciders -------------------------------------------------------------------------------------------------------------
FLT_MIN = np.float32(np.uint32(0x00800000).view(np.float32))
SPECIALS = np.array([0.0, -0.0, DENORM32, -DENORM32, FLT_MIN, -FLT_MIN, np.inf, -np.inf, np.nan, 1.0, -1.0], np.float32)
SPECIALS_POSITIVE = np.array([0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0], bool)     # x > 0, written out (NaN compares false)


def specials_in_noise(n, seed):
    """fp32 [n] random data with the specials scattered through it (the first and the last entry included) -> (x, positions [len(SPECIALS) * reps])"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    reps = 5
    pos = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), len(SPECIALS) * reps - 2, replace=False)])
    x[pos] = np.tile(SPECIALS, reps)
    return x, pos
