"""The power of tests/test_attention_accuracy_gpu.py, proved without a GPU: its metric and bound (tests/_attn_ref.py: row-relative L2 against
float64, bound K_BOUND x the honest bf16 model's own maximum) on its probe inputs, with plain-torch stand-ins in place of the kernel.  The honest
model passes with k = 1; every wrong kernel below — a dropped, doubled, leaked or mis-weighted key — fails at K_BOUND in every case it applies to."""
import pytest
import torch

import _attn_ref as R

torch.set_grad_enabled(False)


def _cases():
    return {
        "noncausal": R.all_rounds(1, 4, 4, 513, 513, 128, seed=1),                                             # test_attention_dma_gpu's list
        "causal_gqa": R.all_rounds(1, 8, 2, 333, 333, 128, causal=True, seed=2),                                # ATT: Llama GQA prefill
        "window": R.all_rounds(1, 4, 4, 700, 700, 96, causal=True, window=100, seed=3),                         # WIN
        "splitkv": R.all_rounds(1, 32, 8, 213, 1697, 128, causal=True, seed=4, split_edges=range(256, 1697, 256)),   # ATT: 8 splits of 256 keys
        "decode": R.decode_rounds(8, 2, 64, 640, 325, seed=5),                                                  # test_decode_attention's list
        "decode_window": R.decode_rounds(4, 4, 96, 1024, 300, window=100, seed=6),                              # test_decode_attention_sliding_window's
    }


CASES = _cases()


def _col(t):
    def edit(vis, i0, i1):
        vis[:, t] = False
    return edit


def _tile(t0):
    def edit(vis, i0, i1):
        vis[:, t0:t0 + 64] = False
    return edit


def _leak63(off):
    def edit(vis, i0, i1):
        for i in range(i0, i1):
            if i % 64 == 63 and i + off + 1 < vis.shape[1]:
                vis[i - i0, i + off + 1] = True
    return edit


def _mutants(case):
    """name -> model keywords (or a case override), for the mutants that apply to this case"""
    Sq, Hq = case["q"].shape[1:3]
    Skv, Hkv = case["k"].shape[1:3]
    causal, window, off = case["causal"], case["window"], Skv - Sq
    first_vis = max(0, Skv - window) if (window and Sq == 1) else 0
    mid = (Skv // 2) // 64 * 64 if Sq > 1 else max(first_vis, (Skv - 1 - (min(window, Skv) if window else Skv) // 2)) // 64 * 64
    boundary = max(64, ((first_vis + Skv) // 2 + 63) // 64 * 64)
    m = {
        "last key dropped": dict(vis_edit=_col(Skv - 1)),
        "last key duplicated": dict(dup_key=Skv - 1),
        "interior 64-key tile dropped": dict(vis_edit=_tile(mid)),
        "scale x 1.02": dict(scale_mul=1.02),
        "split merged with equal weights": dict(split=(boundary, "equal")),
        "split merged without the max rescale": dict(split=(boundary, "norescale")),
    }
    if first_vis == 0:
        m["first key dropped"] = dict(vis_edit=_col(0))
    if causal and Sq > 64:
        m["causal mask leaks diag + 1 at rows = 63 (mod 64)"] = dict(vis_edit=_leak63(off))
    if window:
        m["window one key too long"] = dict(window=window + 1)
        m["window one key too short"] = dict(window=window - 1)
    if Hq > Hkv:
        G = Hq // Hkv
        m["a GQA group on the wrong KV head"] = dict(kv_of_head=[((h // G) + (1 if h // G == 0 else 0)) % Hkv for h in range(Hq)])
    return m


def _stand_in(**kw):
    def kernel(case):
        c = dict(case, window=kw["window"]) if "window" in kw else case
        return R.reference(c, R.attention_bf16_model, **{k: v for k, v in kw.items() if k != "window"})
    return kernel


@pytest.mark.parametrize("name", list(CASES))
def test_honest_model_passes_at_k1(name):
    ek, em = R.evaluate(CASES[name], _stand_in())
    assert R.passes(ek, em, k=1.0)
    assert float(em.max()) < 2e-2          # the bound itself stays a bf16-sized number: K_BOUND x this is far below the O(1) error of a wrong key


@pytest.mark.parametrize("name", list(CASES))
def test_split_merge_with_the_right_weights_passes(name):
    """the two-way split of the mutants below is harmless when merged correctly: what fails there is the merge, not the split"""
    Skv = CASES[name][0]["k"].shape[1]
    ek, em = R.evaluate(CASES[name], _stand_in(split=(max(64, Skv // 2 // 64 * 64), "ok")))
    assert R.passes(ek, em)


@pytest.mark.parametrize("name", list(CASES))
def test_every_mutant_fails_at_the_bound(name):
    rounds = CASES[name]
    survived = []
    for mutant, kw in _mutants(rounds[0]).items():
        ek, em = R.evaluate(rounds, _stand_in(**kw))
        print(f"{name:14s} {mutant:50s} max row err {float(ek.max()):9.3e}  model {float(em.max()):9.3e}  ratio {float(ek.max() / em.max()):8.1f}")
        if R.passes(ek, em):
            survived.append(mutant)
    assert not survived, survived


def test_mutant_list_is_complete():
    names = set()
    for rounds in CASES.values():
        names |= set(_mutants(rounds[0]))
    assert len(names) == 11, sorted(names)


def test_reference_is_the_suite_statement():
    """attention64 states what _cpu_ops.attention states (GQA, shifted diagonal, window), also on a slice of rows"""
    import _cpu_ops as ref
    for (Hq, Hkv, Sq, Skv, causal, window) in ((4, 2, 70, 70, False, 0), (4, 2, 33, 160, True, 0), (4, 4, 150, 200, True, 65)):
        g = torch.Generator().manual_seed(Sq)
        q, k, v = (torch.randn(2, n, h, 32, generator=g).to(torch.bfloat16) for n, h in ((Sq, Hq), (Skv, Hkv), (Skv, Hkv)))
        want = ref.attention(q.float(), k.float(), v.float(), 0.2, causal, window=window).double()
        got, lse = R.attention64(q, k, v, 0.2, causal, window, chunk=32)
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
        part, _ = R.attention64(q[:, 20:31], k, v, 0.2, causal, window, row0=20, Sq_total=Sq)
        torch.testing.assert_close(part, got[:, 20:31], rtol=1e-12, atol=1e-12)
        assert torch.isfinite(lse).all()
