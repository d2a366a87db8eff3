"""return_scores on the CPU statements of the kernels, with the contract's CPU statement (tests/_scores_ref.py) in place of
ops.token_scores_rows: what the three entry points return and in which order, that slot 0 is the prefill's token, EOS truncation,
max_new_tokens = 0, the multi-GPU refusal, chat.py's scores.json, and that the two tools parse --help and stop without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _boxes_ref as BR
import _rle_ref as RR
import _scores_ref as R

torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny():
    import _cpu_ops
    from test_oracle_e2e import e2e_setup
    from videoglamm_amd import _lib, ops
    from videoglamm_amd.model import VideoGLaMMForCausalLM

    with pytest.MonkeyPatch.context() as mp:
        for name in _cpu_ops.ALL:
            if hasattr(ops, name):
                mp.setattr(ops, name, getattr(_cpu_ops, name))
        mp.setattr(ops, "token_scores_rows", R.token_scores_rows)
        mp.setattr(ops, "token_scores_workspace", R.token_scores_workspace)
        mp.setattr(ops, "mask_boxes", BR.mask_boxes)          # return_boxes / return_rle beside return_scores: their CPU statements
        mp.setattr(ops, "mask_rle", RR.mask_rle)
        mp.setattr(_lib, "load", lambda: None)
        fx, sd, cfg, inp = e2e_setup()
        m = VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.float32, device="cpu")
        m.token_hook = lambda step, tok: m.config.seg_token_idx if step == 1 else None
        yield m, inp


def _clip(inp, ids=None):
    ids = inp["input_ids"] if ids is None else ids
    return ([inp["images"]], [inp["context_images"]], [inp["images_for_sam"][:2]], ids[None], [(1024, 1024)], [inp["original_size"]])


def _prompts(inp):
    base = inp["input_ids"]
    n0 = int((base == -200).nonzero().max()) + 1
    return [base, torch.cat([base[:n0], torch.tensor([84, 12, 99, 150, 7])]), torch.cat([base[:n0], torch.tensor([200, 201, 202])])]


def _is_records(s, G):
    assert sorted(s) == ["logprob", "margin", "top2"]
    assert s["logprob"].shape == (G,) and s["logprob"].dtype == np.float32 and s["margin"].shape == (G,) and s["margin"].dtype == np.float32
    assert s["top2"].shape == (G, 2) and s["top2"].dtype == np.int64
    assert np.all(s["margin"] >= 0) and np.all(s["logprob"] <= 0)


def _same_segments(a, b):
    assert sorted(a) == sorted(b)
    for t in a:
        assert sorted(a[t]) == sorted(b[t]) and all(np.array_equal(a[t][k], b[t][k]) for k in a[t])


def _generate(m, inp, n, eos=None, hook=None, ids=None):
    from videoglamm_amd import vlm
    g = torch.Generator().manual_seed(3)
    visual = torch.randn(6, m.cfg["llm"]["hidden"], generator=g) * 0.5
    trace = {"scores": True}
    out, _ = vlm.generate(m.P, m.cfg, None, None, None, inp["input_ids"] if ids is None else ids, n, eos, visual=visual, token_hook=hook, trace=trace)
    return out.tolist(), trace


@pytest.mark.parametrize("video", [False, True])
def test_inference_returns_the_records_last(tiny, video):
    m, inp = tiny
    c = _clip(inp)
    L = c[3].shape[1]
    kw = dict(max_new_tokens=3, use_sam2_video_branch=video)
    ids, segs = m.inference(*c, **kw)
    ids2, segs2, sc = m.inference(*c, return_scores=True, **kw)
    assert torch.equal(ids, ids2) and isinstance(sc, list) and len(sc) == 1
    _same_segments(segs[0], segs2[0])
    _is_records(sc[0], ids.shape[1] - L)
    # slot 0 is the token the prefill emitted; the records are the model's own picks (step 1 was replaced by [SEG])
    assert sc[0]["top2"][0, 0] == int(ids[0, L]) and int(ids[0, L + 1]) == m.config.seg_token_idx
    ids3, segs3, boxes, codes, sc3 = m.inference(*c, return_boxes=True, return_rle=True, return_scores=True, **kw)
    assert torch.equal(ids3, ids) and sorted(boxes[0]) == sorted(codes[0]) == sorted(segs3[0])
    assert all(np.array_equal(sc3[0][k], sc[0][k]) for k in sc[0])
    # capture and scores together: the records reach both
    m.capture = {}
    try:
        _, _, sc4 = m.inference(*c, return_scores=True, **kw)
        assert m.capture["scores"] is sc4[0] and m.capture["argmax"] == sc4[0]["top2"][:, 0].tolist()
    finally:
        m.capture = None


def test_inference_prompts_returns_one_more_list(tiny):
    m, inp = tiny
    ps = _prompts(inp)
    args = ([inp["images"]], [inp["context_images"]], [inp["images_for_sam"][:2]], ps, [(1024, 1024)], [inp["original_size"]])
    out0, segs0 = m.inference_prompts(*args, max_new_tokens=3)
    out, segs, sc = m.inference_prompts(*args, max_new_tokens=3, return_scores=True)
    out2, segs2, boxes2, sc2 = m.inference_prompts(*args, max_new_tokens=3, return_scores=True, return_boxes=True, shared=False)
    assert len(sc) == len(sc2) == len(boxes2) == 3
    for b in range(3):
        assert torch.equal(out[b], out0[b]) and torch.equal(out2[b], out0[b])
        _same_segments(segs[b], segs0[b])
        _is_records(sc[b], out[b].shape[1] - ps[b].numel())
        # the shared route prefills prefix and suffix apart, the per-prompt calls the whole prompt: the same picks, the logits to rounding
        assert np.array_equal(sc[b]["top2"], sc2[b]["top2"])
        assert np.allclose(sc[b]["logprob"], sc2[b]["logprob"], atol=1e-4) and np.allclose(sc[b]["margin"], sc2[b]["margin"], atol=1e-4)
        assert sc[b]["top2"][0, 0] == int(out[b][0, ps[b].numel()])
        assert sorted(boxes2[b]) == sorted(segs2[b])


def test_inference_clips_returns_one_more_element(tiny):
    m, inp = tiny
    cl = [_clip(inp, ids) for ids in _prompts(inp)[:2]]
    plain = m.inference_clips(cl, max_new_tokens=3)
    got = m.inference_clips(cl, max_new_tokens=3, return_rle=True, return_scores=True)
    for (o, s), (o2, s2, codes, sc), c in zip(plain, got, cl):
        assert torch.equal(o, o2) and len(sc) == 1 and sorted(codes[0]) == sorted(s2[0])
        _same_segments(s[0], s2[0])
        _is_records(sc[0], o.shape[1] - c[3].shape[1])
        ref = m.inference(*c, max_new_tokens=3, return_scores=True)[-1]
        assert all(np.array_equal(sc[0][k], ref[0][k]) for k in ref[0])


def test_records_follow_the_loop(tiny):
    """slot j describes the logits that emitted token j; an EOS cuts the records with the ids; max_new_tokens = 0 gives empty arrays"""
    m, inp = tiny
    L = inp["input_ids"].numel()
    out, tr = _generate(m, inp, 5)
    G = len(out) - L
    assert G == 5 and tr["argmax"] == out[L:] == tr["scores"]["top2"][:, 0].tolist()
    _is_records(tr["scores"], G)
    # against the statement applied to the logits of the emitting rows
    dec = m.P._decoder
    S = dec.pos - (G - 1)
    for j in range(G):
        logits = dec.proj.lm_head(False, m.P, dec.hid_all[S - 1 + j:S + j])
        lp, mg, t2 = R.reference(logits.view(1, -1), [out[L + j]])
        assert np.float32(lp[0]) == tr["scores"]["logprob"][j] and mg[0] == tr["scores"]["margin"][j] and t2[0].tolist() == tr["scores"]["top2"][j].tolist()
    # EOS = the third generated id: three records
    eos = out[L + 2]
    first = out[L:].index(eos)
    out_e, tr_e = _generate(m, inp, 5, eos=eos)
    assert len(out_e) - L == first + 1
    _is_records(tr_e["scores"], first + 1)
    assert all(np.array_equal(tr_e["scores"][k], tr["scores"][k][:first + 1]) for k in tr["scores"])
    # a forced token does not change what the record describes
    out_f, tr_f = _generate(m, inp, 2, hook=lambda step, tok: 9 if step == 0 else None)
    assert out_f[L] == 9 and tr_f["scores"]["top2"][0, 0] == out[L] and tr_f["scores"]["logprob"][0] == tr["scores"]["logprob"][0]
    out_0, tr_0 = _generate(m, inp, 0)
    assert len(out_0) == L
    _is_records(tr_0["scores"], 0)
    # a trace that does not ask gets nothing, and the decoder's step is the one without the launch
    from videoglamm_amd import vlm
    plain = {}
    vlm.generate(m.P, m.cfg, None, None, None, inp["input_ids"], 2, None, visual=torch.zeros(6, m.cfg["llm"]["hidden"]), trace=plain)
    assert "scores" not in plain and m.P._decoder.scores_on is False


def test_multi_gpu_refusal_comes_before_any_work(tiny):
    m, inp = tiny

    class World:
        def __init__(self, world):
            self.world = world

    try:
        m.comm = World(2)
        with pytest.raises(NotImplementedError, match="return_scores"):
            m.inference(None, None, None, None, None, None, return_scores=True)
        with pytest.raises(NotImplementedError, match="return_scores"):
            m.inference(None, None, None, None, None, None, use_sam2_video_branch=True, return_scores=True)
        m.comm = World(1)                   # (a world of 2 is refused by the two batched entry points whatever the keywords)
        with pytest.raises(NotImplementedError, match="return_scores"):
            m.inference_prompts(None, None, None, None, None, None, return_scores=True)
        with pytest.raises(NotImplementedError, match="return_scores"):
            m.inference_clips(None, return_scores=True)
    finally:
        m.comm = None


def test_chat_writes_scores_json(tmp_path, monkeypatch):
    from videoglamm_amd import chat
    monkeypatch.setattr(sys, "argv", ["chat.py", "--llava_version_or_path", "x", "--save_scores"])
    assert chat.get_args().save_scores is True
    monkeypatch.setattr(sys, "argv", ["chat.py", "--llava_version_or_path", "x"])
    assert chat.get_args().save_scores is False
    scores = {"logprob": np.array([-0.5, float("nan"), -2.25], np.float32), "margin": np.array([1.5, 0.0, 0.125], np.float32),
              "top2": np.array([[7, 3], [4, 9], [11, 12]], np.int64)}
    chat.write_scores(torch.tensor([[1, 2, 3, 7, 5, 11]]).numpy(), scores, str(tmp_path))
    rows = json.load(open(tmp_path / "scores.json"))
    assert rows == [{"id": 7, "logprob": -0.5, "margin": 1.5, "top1": 7, "runner_up": 3},
                    {"id": 5, "logprob": None, "margin": 0.0, "top1": 4, "runner_up": 9},
                    {"id": 11, "logprob": -2.25, "margin": 0.125, "top1": 11, "runner_up": 12}]
    chat.write_scores(np.array([[1, 2]]), {"logprob": np.zeros(0, np.float32), "margin": np.zeros(0, np.float32), "top2": np.zeros((0, 2), np.int64)},
                      str(tmp_path))
    assert json.load(open(tmp_path / "scores.json")) == []


@pytest.mark.parametrize("tool", ["bench_scores.py", "decode_margins.py"])
def test_tools_parse_help_and_stop_without_a_gpu(tool):
    path = os.path.join(ROOT, "tools", tool)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")         # no device for the tool, wherever the test runs
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "--out" in r.stdout
    r = subprocess.run([sys.executable, path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "no GPU" in r.stderr and not r.stdout.strip()
