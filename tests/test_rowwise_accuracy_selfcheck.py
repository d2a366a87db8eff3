"""The power of tests/test_rowwise_accuracy_gpu.py, proven on the CPU (no GPU, not marked gpu).

The checks of tests/_rowwise_ref.py run here on CPU stand-ins for the kernels:
  * honest fp32 models pass every case: torch's fp32 statements (tests/_cpu_ops.py), a transcription of norm_short_kernel's lane-strided sums and
    butterfly (norm_lanes_fp32) and a transcription of vg_gelu_erf (gelu_device_fp32);
  * each wrong kernel fails at least one case of every shape class it applies to (the classes below: one per route family of launch_norm_t and per
    dtype pair; a padded divisor applies where the padded width differs from C, the one-pass variance and the forgotten b to LayerNorm);
  * the composed cases (the one-hot vg_mlp_rows model, a column-picked prologue, axpby, the sigmoid mask) have honest and wrong stand-ins too.
The wrong kernels are those listed in the GPU test's docstring.
"""
import pytest
import torch

import _rowwise_ref as R

BF, F32 = R.BF, R.F32
torch.set_grad_enabled(False)

# (name, input dtype, output dtype, rows, C, TPR, NV): the lane geometry of the route the shape takes in vg_rowops.hip
CLASSES = [
    ("scalar C=4", BF, BF, 5, 4, 256, 1),
    ("norm_short<8,3> C=144", BF, BF, 120, 144, 8, 8),
    ("one wave per row, misaligned C=520", BF, BF, 80, 520, 64, 8),
    ("norm_short<64,3> C=1408", BF, BF, 60, 1408, 64, 8),
    ("norm_short<64,8> C=4096", BF, BF, 44, 4096, 64, 8),
    ("16 lanes per row, bf16 -> fp32 C=288", BF, F32, 100, 288, 16, 8),
    ("one wave per row, fp32 C=260", F32, F32, 80, 260, 64, 4),
    ("workgroup per row, fp32 -> bf16 C=2048", F32, BF, 48, 2048, 256, 4),
]


def _norm_cases(cls, rms, has_w=True):
    """[(case, x, w, b, eps)] over the rounds of a class"""
    name, dt, odt, rows, C, tpr, nv = cls
    w, b = R.norm_weights(C) if has_w else (None, None)
    b = None if rms else b
    eps = 1e-5 if rms else 1e-6
    out = []
    for x, probes in R.build_norm_rounds(rows, C, dt, rms, tpr, nv, seed=1):
        out.append((R.norm_case(f"{'rms' if rms else 'ln'} {name}", x, w, b, eps, rms, odt, probes=probes), x, w, b, eps))
    return out


def _run(cls, rms, mutant, has_w=True):
    """the verdict over all rounds together, as the GPU test forms it"""
    name, dt, odt, rows, C, tpr, nv = cls
    cs = _norm_cases(cls, rms, has_w)
    got = torch.cat([R.norm_lanes_fp32(x, w, b, eps, rms, tpr, nv, mutant).to(odt).reshape(-1) for _, x, w, b, eps in cs])
    whole = R.cat_cases(cs[0][0].name, [c for c, *_ in cs])
    whole.precondition()
    return whole.evaluate(got)


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c[0])
def test_honest_norm_models_pass(cls):
    name, dt, odt, rows, C, tpr, nv = cls
    for rms in (False, True):
        cs = _norm_cases(cls, rms)
        whole = R.cat_cases(cs[0][0].name, [c for c, *_ in cs])
        whole.precondition()
        r = whole.evaluate(whole.cpu32.to(odt))                     # torch's fp32 statement
        assert r["ok"], ("statement", name, rms, r)
        r = _run(cls, rms, None)                                     # the lane-strided transcription
        print(R.line(whole, r))
        assert r["ok"], ("lanes", name, rms, r)


def _applies(mutant, cls, rms):
    name, dt, odt, rows, C, tpr, nv = cls
    if mutant == "divisor padded to the lane width":
        return C % (tpr * nv) != 0
    if mutant == "one-pass fp32 variance":
        # (bf16 rows shorter than 64: x^2 has 16 bits and a row's sum of squares fewer than 24, so E[x^2] - mean^2 is exact in fp32 — not a wrong kernel)
        return not rms and not (dt == BF and C < 64)
    if mutant == "last 8-column chunk dropped":
        return nv > 1
    if mutant in R.RMS_MUTANTS:
        return rms and (mutant != "RMSNorm without the intermediate rounding" or dt == BF)
    if mutant in R.LN_MUTANTS:
        return not rms
    return True


@pytest.mark.parametrize("mutant", R.NORM_MUTANTS + R.RMS_MUTANTS + R.LN_MUTANTS)
def test_wrong_norm_kernels_fail(mutant):
    seen = 0
    for cls in CLASSES:
        for rms in (False, True):
            if not _applies(mutant, cls, rms):
                continue
            # a mutant that touches the statistics must show in LayerNorm AND in RMSNorm of every class; the others have one form only
            r = _run(cls, rms, mutant)
            assert not r["ok"], (mutant, cls[0], "rms" if rms else "ln", r)
            seen += 1
    assert seen >= 3, mutant


@pytest.mark.parametrize("cls", [CLASSES[1], CLASSES[4]], ids=lambda c: c[0])
def test_weightless_norm_cases(cls):
    """without w and b the share counts each distinct value of a row once and the element check carries the power: the honest kernel passes, and
    eps x 10 (share below the cap) and a dropped column fail, in LayerNorm and RMSNorm"""
    for rms in (False, True):
        assert _run(cls, rms, None, has_w=False)["ok"]
        for mutant in ("eps x 10", "last column dropped from the statistics", "divisor C - 1"):
            r = _run(cls, rms, mutant, has_w=False)
            assert not r["ok"] and r["bad"] > 0, (mutant, rms, r)


# ------------------------------------------------------------------ activations
@pytest.mark.parametrize("dt,odt", [(BF, BF), (F32, F32), (BF, F32)], ids=["bf16", "fp32", "bf16-fp32"])
def test_activation_models(dt, odt):
    x = R.act_grid(dt)
    for act in (1, 2, 3, 4, 5):
        c = R.act_case(f"act {act}", x, act, odt)
        c.precondition()
        r = c.evaluate(c.cpu32.to(odt))
        assert r["ok"], ("statement", act, r)
    c = R.act_case("gelu", x, R.ACT_GELU, odt)
    r = c.evaluate(R.gelu_device_fp32(x).to(odt))
    print(R.line(c, r))
    assert r["ok"], ("vg_gelu_erf transcription", r)
    r = c.evaluate(R.gelu_tanh_fp32(x).to(odt))
    assert not r["ok"], ("tanh GELU", r)
    if odt == BF:          # the bf16-only paths: the share check alone must see it (the largest difference is a tenth of a bf16 step)
        assert r["share"] > r["cap"], r
    c = R.act_case("quick", x, R.ACT_QUICK_GELU, odt)
    assert not c.evaluate(R.quick_gelu_17_fp32(x).to(odt))["ok"], "quick-GELU with 1.7 for 1.702"


def _gu(dt):
    g = torch.Generator().manual_seed(5)
    gu = torch.randn(64, 2 * 96, generator=g) * 2.0
    gu[0, :8] = torch.tensor([0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0])
    return gu.to(dt)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_swiglu_models(dt):
    gu = _gu(dt)
    c = R.swiglu_case("swiglu", gu)
    c.precondition()
    assert c.evaluate(R.swiglu_fp32(gu).to(dt))["ok"]
    assert not c.evaluate(R.swiglu_fp32(gu, "SwiGLU with gate and up swapped").to(dt))["ok"]
    if dt == BF:
        assert not c.evaluate(R.swiglu_fp32(gu, "SwiGLU without the bf16 rounding of the gate").to(dt))["ok"]


def test_mlp_onehot_model():
    """mlp_onehot_case (vg_mlp_rows under one-hot weights): torch's statement and the pipeline with the device GELU pass; tanh GELU, eps x 10, a
    skipped rounding of the LayerNorm output and a column dropped from the statistics fail"""
    import torch.nn.functional as F
    C, M = 144, 100
    lw, lb = R.norm_weights(C)
    lw, lb = 1.0 + 0.1 * lw, 0.1 * lb
    x, probes = R.build_norm_rounds(M, C, BF, False, 8, 8, seed=9)[0]
    c = R.mlp_onehot_case("mlp_rows one-hot", x, lw, lb, 1e-6, probes)
    c.precondition()

    def pipe(gelu=R.gelu_device_fp32, mutant=None, round_ln=True):
        n = R.norm_lanes_fp32(x, lw, lb, 1e-6, False, 8, 8, mutant)
        n = n.to(BF).float() if round_ln else n
        return (x.float() + gelu(n).to(BF).float()).to(BF)
    assert c.evaluate(c.cpu32.to(BF))["ok"]
    assert c.evaluate(pipe())["ok"]
    assert c.evaluate(pipe(gelu=F.gelu))["ok"]
    assert not c.evaluate(pipe(gelu=R.gelu_tanh_fp32))["ok"]
    assert not c.evaluate(pipe(mutant="eps x 10"))["ok"]
    assert not c.evaluate(pipe(mutant="last column dropped from the statistics"))["ok"]
    assert not c.evaluate(pipe(round_ln=False))["ok"]


def test_column_picked_prologue_model():
    """the prologue cases of the GPU test: an RMSNorm case restricted to the columns a one-hot W picks (a decode row of K = 3072, 256 lanes of 8)"""
    K, N = 3072, 256
    pi = torch.cat([torch.tensor([c for e in R.spike_columns(K, 256, 8) for c in (e - 1, e, e + 1) if 0 <= c < K]).unique(), torch.arange(5, K, 13)])[:N]
    nw = R.norm_weights(K)[0]
    cases, xs = [], []
    for x, probes in R.build_norm_rounds(16, K, BF, True, 256, 8, seed=20):
        full = R.norm_case("prologue", x, nw, None, 1e-5, True, BF, probes=probes)
        pick = lambda t: t[:, pi]                                                                       # noqa: E731
        cases.append(R.Case("prologue", [pick(r) for r in full.refs], [pick(u) for u in full.units], BF, cpu32=pick(full.cpu32), counted=pick(full.counted)))
        xs.append(x)
    whole = R.cat_cases("prologue", cases)
    whole.precondition()
    run = lambda m: torch.cat([R.norm_lanes_fp32(x, nw, None, 1e-5, True, 256, 8, m).to(BF)[:, pi].reshape(-1) for x in xs])      # noqa: E731
    assert whole.evaluate(run(None))["ok"]
    for m in ("last column dropped from the statistics", "last 8-column chunk dropped", "one column counted twice", "divisor C - 1", "eps x 10",
              "RMSNorm without the intermediate rounding", "RMSNorm that subtracts a mean"):
        assert not whole.evaluate(run(m))["ok"], m


def test_axpby_and_mask_models():
    """axpby_case (element check, fixed multiple 2) and mask_sigmoid_case: the fp32 statements pass; a swapped alpha / beta, a dropped beta term and a
    mask scale applied after the bias fail"""
    g = torch.Generator().manual_seed(13)
    for dt in (BF, F32):
        a, b = (torch.randn(6, 50, 32, generator=g) * 3.0).to(dt), torch.randn(50, 32, generator=g).to(dt)
        bb = b.repeat(6, 1, 1)
        c = R.axpby_case("axpby", a, b, 0.5, -1.5, dt)
        assert c.evaluate((0.5 * a.float() + -1.5 * bb.float()).to(dt))["ok"]
        assert not c.evaluate((-1.5 * a.float() + 0.5 * bb.float()).to(dt))["ok"]
        assert not c.evaluate((0.5 * a.float()).to(dt))["ok"]
        x = torch.cat([R.act_grid(F32)[:24000], torch.randn(4800, generator=g) * 4.0])
        c = R.mask_sigmoid_case("mask", x, 20.0, -10.0, dt)
        c.precondition()
        assert c.evaluate((torch.sigmoid(x) * 20.0 - 10.0).to(dt))["ok"]
        assert not c.evaluate(((torch.sigmoid(x) - 10.0) * 20.0).to(dt))["ok"]
        assert not c.evaluate(((x > 0).float() * 20.0 - 10.0).to(dt))["ok"]


# ------------------------------------------------------------------ rotations
def _tables(n, hd, seed):
    g = torch.Generator().manual_seed(seed)
    ang = torch.randn(n, hd, generator=g) * 2.0
    return ang.cos(), ang.sin()


def test_rope_half_models():
    import _cpu_ops as ref
    cos, sin = _tables(60, 16, 1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(37, 3, 32, generator=g).to(BF)
    want = R.rope_half_bf16(x, cos, sin, 11)
    assert torch.equal(ref.rope_half_(x.clone(), cos, sin, 11), want)                              # the suite's bf16 statement is this arithmetic
    assert not torch.equal(R.rope_half_bf16(x, cos, sin, 11, fp32_products=True), want)           # rope_half with fp32 products
    assert not torch.equal(R.rope_half_bf16(x, cos, sin, 11, flip_sin_half=True), want)           # the sign of sin flipped on one half
    xf = torch.randn(37, 3, 32, generator=g)
    c = R.rope_half_case("rope_half fp32", xf, cos, sin, 11)
    assert c.evaluate(ref.rope_half_(xf.clone(), cos, sin, 11))["ok"]
    bad = ref.rope_half_(xf.clone(), cos, -sin, 11)
    bad[..., :16] = ref.rope_half_(xf.clone(), cos, sin, 11)[..., :16]
    assert not c.evaluate(bad)["ok"]


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_rope_axial_models(dt):
    n_grid, n_rope, C = 16, 32, 32
    cos, sin = _tables(n_rope, C // 2, 3)          # (rows past n_grid exist for the wrong kernel to read)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, n_rope + 5, C, generator=g).to(dt)
    c = R.rope_axial_case("rope_axial", x, cos, sin, n_rope, n_grid)
    c.precondition()
    assert c.evaluate(R.rope_axial_fp32(x, cos, sin, n_rope, n_grid).to(dt))["ok"]
    assert not c.evaluate(R.rope_axial_fp32(x, cos, sin, n_rope, n_grid, "table row of tok").to(dt))["ok"]


def test_formats():
    """round_to is one rounding to nearest even from float64, and quantum the spacing it uses"""
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.0, 0.0, 2.0 ** -130, 255.5], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0, 2.0 ** -130, 256.0]).to(BF)
    assert torch.equal(R.round_to(v, BF), want)
    assert torch.equal(R.round_to(v, F32), v.float())
    f = torch.randn(4096, dtype=torch.float64)
    assert torch.equal(R.round_to(f, F32), f.float())
    assert torch.equal(R.round_to(f.float().double(), BF), f.float().to(BF))
