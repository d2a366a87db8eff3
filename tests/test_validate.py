"""The validation metrics gIoU / cIoU without a GPU (tests/golden/validate.npz holds what the reference's own
intersectionAndUnionGPU, AverageMeter and validator statements gave, tests/golden/make_golden_validate.py): the numpy statement
of the kernel's contract against the reference's per-frame triples, the host arithmetic of postproc.record_from_counts /
ValidationMeter against its records and its (giou, ciou) bit for bit, the refusals that come before any GPU work, and a
self-check: the fixture's inputs tell five deliberate defects of the statement from the statement."""
import numpy as np
import pytest
import torch

import _validate_ref as R

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def _ignore(fx):
    return int(fx["ignore_index"])


def test_statement_equals_the_reference_triples(fx):
    for name in ("s0", "s1", "s2", "one"):
        x, t, want = fx[f"{name}_logits"], fx[f"{name}_target"], fx[f"{name}_triples"]
        inter, union, tgt = R.triples(R.counts(x, t, _ignore(fx)))
        assert np.array_equal(np.stack([inter, union, tgt], 1), want), name


def test_fixture_holds_the_cases_it_is_meant_to(fx):
    x0, t0 = R.sample_frames(fx, 0)
    assert [fx[f"s{s}_logits"].shape for s in range(3)] == [(3, 37, 53), (4, 37, 53), (5, 37, 53)]
    assert fx["one_logits"].shape[1:] == (1, 1)
    assert (fx["s0_triples"][1, 1, 1] == 0) and (fx["s0_triples"][1, 1, 0] > 0)          # frame 1 of sample 0: union[1] == 0 only
    assert (t0[2] == _ignore(fx)).all() and (fx["s0_triples"][2] == 0).all()             # frame 2: all ignore, every count 0
    assert (fx["s1_target"] == 7).any()
    seen = np.concatenate([fx[f"s{s}_logits"].ravel() for s in range(3)])
    assert np.isnan(seen).any() and np.isposinf(seen).any() and np.isneginf(seen).any()
    assert ((seen == 0) & ~np.signbit(seen)).any() and ((seen == 0) & np.signbit(seen)).any()
    assert (seen == np.float32(1e-45)).any() and np.float32(1e-45) > 0
    assert max(int(fx[f"s{s}_triples"].max()) for s in range(3)) < 2 ** 24


def test_record_and_meter_equal_the_reference_bit_for_bit(fx):
    from videoglamm_amd import postproc

    meter = postproc.ValidationMeter()
    for s in range(3):
        x, t = R.sample_frames(fx, s)
        rec = postproc.record_from_counts(R.counts(x, t, _ignore(fx)))
        for got, key in zip(rec[:3], ("intersection", "union", "acc_iou")):
            want = fx[f"s{s}_{key}"]
            assert got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes(), (s, key, got, want)
        assert rec[3] == int(fx[f"s{s}_n"])
        # [1, T, 6] is the same sample, and [2, T, 6] enters the 2 T rows alike with n = 2 T
        again = postproc.record_from_counts(R.counts(x[None], t[None], _ignore(fx)))
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], rec[:3])) and again[3] == rec[3]
        twice = postproc.record_from_counts(R.counts(np.stack([x, x]), np.stack([t, t]), _ignore(fx)))
        assert twice[3] == 2 * rec[3] and np.array_equal(twice[0], 2 * rec[0]) and np.array_equal(twice[1], 2 * rec[1])
        meter.update(rec)
    giou, ciou = meter.result()
    assert isinstance(giou, float) and isinstance(ciou, float)
    assert np.float32(giou).tobytes() == fx["giou"].tobytes() and np.float32(ciou).tobytes() == fx["ciou"].tobytes()
    assert giou == float(fx["giou"]) and ciou == float(fx["ciou"])
    with pytest.raises(ValueError):
        postproc.ValidationMeter().result()


def _twin(monkeypatch):
    """the operator replaced by its numpy statement; device uploads switched off"""
    from videoglamm_amd import ops, postproc

    monkeypatch.setattr(ops, "logit_class_counts", R.logit_class_counts, raising=True)
    monkeypatch.setattr(postproc, "_dev", lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)))
    return postproc


def test_reference_name_and_record_on_the_twin(fx, monkeypatch):
    postproc = _twin(monkeypatch)
    ign = _ignore(fx)
    for s in range(3):
        x, t = R.sample_frames(fx, s)
        with np.errstate(invalid="ignore"):
            labels = torch.from_numpy((x > 0).astype(np.float32))
        for f in range(x.shape[0]):                                   # the reference's name, per frame, float and integer labels
            for out, tgt in ((labels[f], torch.from_numpy(t[f].astype(np.float32))), (labels[f].int(), torch.from_numpy(t[f]).int())):
                before = out.clone()
                got = postproc.intersectionAndUnionGPU(out, tgt, 2, ignore_index=ign)
                assert all(g.dtype == torch.float32 and g.shape == (2,) for g in got)
                assert np.array_equal(np.stack([g.numpy() for g in got]), fx[f"s{s}_triples"][f].astype(np.float32))
                assert torch.equal(out, before)                       # no write into `output`
        out = {"pred_masks": [[torch.from_numpy(x[f])[None] for f in range(x.shape[0])]], "gt_masks": [torch.from_numpy(t)[None]]}
        rec = postproc.validation_record(out, ign)
        for got, key in zip(rec[:3], ("intersection", "union", "acc_iou")):
            assert got.tobytes() == fx[f"s{s}_{key}"].tobytes(), (s, key)
        # no [SEG]: [0, H, W] per frame counts as all-background logits
        none = {"pred_masks": [[torch.zeros(0, *x.shape[1:]) for _ in range(x.shape[0])]], "gt_masks": [torch.from_numpy(t)[None]]}
        want = postproc.record_from_counts(R.counts(np.zeros_like(x), t, ign))
        assert all(np.array_equal(a, b) for a, b in zip(postproc.validation_record(none, ign)[:3], want[:3]))
    empty = postproc.intersectionAndUnionGPU(torch.zeros(0), torch.zeros(0), 2)
    assert all(torch.equal(e, torch.zeros(2)) for e in empty)


def test_refusals_come_before_any_gpu_work(monkeypatch):
    from videoglamm_amd import ops, postproc
    from videoglamm_amd.model import VideoGLaMMForCausalLM

    def boom(*a, **k):
        raise AssertionError("GPU work was reached")

    monkeypatch.setattr(ops, "logit_class_counts", boom, raising=True)
    monkeypatch.setattr(postproc, "_dev", boom)
    a = torch.zeros(4, 5)
    for K in (1, 3, 19):
        with pytest.raises(NotImplementedError):
            postproc.intersectionAndUnionGPU(a, a, K)
    with pytest.raises(AssertionError, match="^$"):
        postproc.intersectionAndUnionGPU(a, torch.zeros(5, 4), 2)             # the reference's own assert
    with pytest.raises(AssertionError, match="^$"):
        postproc.intersectionAndUnionGPU(torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3, 4), 2)
    for p, g in ((torch.zeros(2, 4, 5), torch.zeros(2, 5, 4)), (torch.zeros(4, 5), torch.zeros(4, 5)), (torch.zeros(1, 2, 4, 5), torch.zeros(2, 4, 5))):
        with pytest.raises(ValueError):
            postproc.validation_counts(p, g)
    m = object.__new__(VideoGLaMMForCausalLM)                        # validate() looks at comm before anything else
    m.comm = object()
    m.model_forward = boom

    def samples():
        raise AssertionError("the samples were touched")
        yield

    with pytest.raises(NotImplementedError, match="one GPU"):
        m.validate(samples())


def check_validate_end_to_end(device, shifts=(1, -2)):
    """the tiny synthetic model of tests/test_facade.py: model_forward(inference=True) with a ground truth that carries an ignore
    band -> validation_record == the host arithmetic on the statement's counts of the downloaded logits; validate() over two
    samples == the meter fed by hand.  Shared with tests/test_validate_gpu.py."""
    from test_facade import build
    from videoglamm_amd import postproc as PP

    fx, inp, m = build(device)
    hw = inp["original_size"]
    ref = torch.from_numpy(fx["framewise_masks"].numpy() > 0.5).permute(1, 0, 2, 3).contiguous()       # [N, T, H, W]
    kw = dict(images_for_sam=[inp["images_for_sam"]], images=[inp["images"]], context_images=[inp["context_images"]],
              input_ids=fx["framewise_output_ids"].long()[None], label_list=[torch.zeros(hw)])
    samples, records = [], []
    for shift in shifts:
        gt = torch.roll(ref, shifts=(shift, 2 * shift), dims=(-2, -1)).to(torch.uint8)
        gt[..., :, -3:] = 255                                        # an ignore band over every frame
        gt[..., 0, :] = 255
        samples.append(dict(kw, masks_list=[gt.to(device)]))
        out = m.model_forward(**samples[-1], inference=True)
        logits = torch.stack([x.float().cpu() for x in out["pred_masks"][0]]).permute(1, 0, 2, 3)     # [N, T, H, W]
        assert logits.shape == gt.shape and logits.shape[0] >= 1
        rec = PP.validation_record(out)
        want = PP.record_from_counts(R.counts(logits.numpy(), gt.numpy(), 255))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rec[:3], want[:3])) and rec[3] == want[3] == gt.shape[0] * gt.shape[1]
        assert rec[1][1] > 0                                         # the sample says something: class 1 has pixels
        records.append(rec)
    assert len(records) < 2 or not np.array_equal(records[0][0], records[1][0])          # and the samples differ
    for n in sorted({len(records), 1}, reverse=True):
        meter = PP.ValidationMeter()
        for rec in records[:n]:
            meter.update(rec)
        assert m.validate(iter(samples[:n])) == meter.result()


def test_validate_end_to_end_cpu(cpu_ops, monkeypatch):
    from videoglamm_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: None)
    _twin(monkeypatch)
    check_validate_end_to_end(torch.device("cpu"), shifts=(1,))          # one sample: the forward passes are slow on the CPU twins


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_fixture_tells_every_mutant_from_the_statement(fx, mutant):
    ign = _ignore(fx)
    changed = 0
    for name in ("s0", "s1", "s2", "one"):
        x, t = fx[f"{name}_logits"], fx[f"{name}_target"]
        changed += int((R.counts(x, t, ign, mutant=mutant) != R.counts(x, t, ign)).sum())
    assert changed > 0, mutant


def test_mutants_are_distinct_defects(fx):
    """no two mutants give the same tables on the fixture: each check above is about its own defect"""
    ign = _ignore(fx)
    tabs = {m: np.concatenate([R.counts(fx[f"{n}_logits"], fx[f"{n}_target"], ign, mutant=m).ravel() for n in ("s0", "s1", "s2", "one")])
            for m in R.MUTANTS}
    names = list(tabs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(tabs[a], tabs[b]), (a, b)
