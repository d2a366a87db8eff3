"""Sampled decoding on the host side (no GPU): the CPU statement of the warpers against transformers' own, the numpy Philox against the published
known-answer vectors, generation_config.json ingest, the keyword > model.generation_config > checkpoint precedence, refusals, seeding, and
the multi-rank seed broadcast (world-2 gloo)."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _cpu_sampling as S

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("T,k,p", [(1.0, 50, 1.0), (0.6, 50, 0.9), (1.7, 0, 0.9), (0.3, 5, 1.0), (1.0, 0, 1.0), (1.0, 10 ** 6, 0.5),
                                   (1.0, 1, 1.0), (0.6, 0, 1e-4)])
def test_cpu_statement_equals_transformers_warpers(T, k, p):
    tr = pytest.importorskip("transformers")
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 3000, generator=g) * 3
    x[0, 100:140] = x[0].max() - 0.5           # 40 ties at a high value: the k-th value falls inside them for k = 5 / 10 / 50
    ids = torch.zeros(1, 1, dtype=torch.int64)
    want = x.clone()
    if T != 1.0:
        want = TemperatureLogitsWarper(T)(ids, want)
    if k != 0:
        want = TopKLogitsWarper(top_k=k)(ids, want)
    if p < 1.0:
        want = TopPLogitsWarper(top_p=p)(ids, want)
    got = S.hf_warp(x, T, k, p)
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isfinite(got)], want[torch.isfinite(want)])
    # the float64 kept set of the contract: the same survivors (ties at the k-th value all kept, the top-p cut away from an edge here)
    order, prob, margin = S.kept(x[0].numpy(), T, k, p)
    keep = torch.isfinite(want[0])
    y = x[0] / T if T != 1.0 else x[0]
    cut_tied = p < 1.0 and bool((y[~keep] == y[keep].min()).any())     # a top-p cut inside a run of ties: HF's order there is torch.sort's
    if not cut_tied:
        assert sorted(order.tolist()) == keep.nonzero().flatten().tolist()
    else:
        assert len(order) == int(keep.sum())
    assert abs(prob.sum() - 1) < 1e-12
    if k == 5:
        assert len(order) == 41                             # the max + 40 ties at the 5th value: ties at the threshold survive together
    if p == 1e-4:
        assert len(order) == 1


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = S.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert [int(v) for v in got] == list(want)
    u = [S.uniform(1234, s) for s in range(1000)]
    assert all(0 <= v < 1 for v in u) and 0.45 < np.mean(u) < 0.55


def test_generation_settings_ingest(tmp_path):
    from videoglamm_amd import ingest
    assert ingest.generation_settings(None) == dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0)
    assert ingest.generation_settings({"eos_token_id": [7, 9]})["do_sample"] is False      # EOS ids only: greedy
    g = ingest.generation_settings({"do_sample": True, "temperature": 0.6, "top_p": 0.9, "eos_token_id": 1, "repetition_penalty": 1.2})
    assert g == dict(do_sample=True, temperature=0.6, top_k=50, top_p=0.9, repetition_penalty=1.2)
    # through the released-directory reader
    from test_oracle_e2e import e2e_setup
    from test_ingest import write_released
    fx, sd, cfg, inp = e2e_setup()
    model_dir = write_released(tmp_path, sd, cfg, "bin")
    got, hf = ingest.load_state_dict(str(model_dir), sam2_checkpoint=str(tmp_path / "sam2_hiera.pt"))
    assert ingest.derive_config(got, hf, seg_token_idx=300)["generation"]["do_sample"] is False       # no generation_config.json
    json.dump({"do_sample": True, "temperature": 0.6, "top_k": 20, "top_p": 0.9, "eos_token_id": [7]}, open(model_dir / "generation_config.json", "w"))
    got, hf = ingest.load_state_dict(str(model_dir), sam2_checkpoint=str(tmp_path / "sam2_hiera.pt"))
    c = ingest.derive_config(got, hf, seg_token_idx=300)
    assert c["generation"] == dict(do_sample=True, temperature=0.6, top_k=20, top_p=0.9) and c["eos_token_id"] == [7]


def test_precedence_refusals_and_seeding():
    from videoglamm_amd.model import GenerationConfig, resolve_sampling
    ckpt = GenerationConfig(dict(do_sample=True, temperature=0.6, top_k=20, top_p=0.9))
    assert GenerationConfig().do_sample is False and resolve_sampling(GenerationConfig()) is None
    s = resolve_sampling(ckpt)
    assert (s["T"], s["k"], s["p"]) == (0.6, 20, 0.9)
    ckpt.temperature = 1.3                                  # model.generation_config assignment beats the checkpoint
    assert resolve_sampling(ckpt)["T"] == 1.3
    s = resolve_sampling(ckpt, temperature=0.5, top_k=0, top_p=1.0)     # keywords beat model.generation_config
    assert (s["T"], s["k"], s["p"]) == (0.5, 0, 1.0)
    assert resolve_sampling(ckpt, do_sample=False) is None
    assert resolve_sampling(GenerationConfig(), do_sample=True)["k"] == 50     # HF's defaults: top_k 50, T 1, p 1
    with pytest.raises(ValueError):
        resolve_sampling(ckpt, temperature=0.0)
    with pytest.raises(ValueError):
        resolve_sampling(ckpt, top_p=1.5)
    for field, v in [("repetition_penalty", 1.1), ("no_repeat_ngram_size", 3), ("typical_p", 0.9), ("min_p", 0.05), ("epsilon_cutoff", 3e-4),
                     ("eta_cutoff", 1e-3), ("num_beams", 4)]:
        bad = GenerationConfig(dict(do_sample=True, **{field: v}))
        with pytest.raises(NotImplementedError, match=field):
            resolve_sampling(bad)
        assert resolve_sampling(bad, do_sample=False) is None        # greedy runs are not refused
    # torch.manual_seed reproduces; a generator is honoured; greedy leaves the RNG alone
    torch.manual_seed(7)
    a = resolve_sampling(ckpt)["seed"]
    torch.manual_seed(7)
    b = resolve_sampling(ckpt)["seed"]
    c = resolve_sampling(ckpt)["seed"]
    assert a == b != c
    assert resolve_sampling(ckpt, generator=torch.Generator().manual_seed(3))["seed"] == \
        resolve_sampling(ckpt, generator=torch.Generator().manual_seed(3))["seed"]
    torch.manual_seed(7)
    resolve_sampling(ckpt, do_sample=False)
    assert resolve_sampling(ckpt)["seed"] == a


def _seed_worker(rank, world, port, q):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch.distributed as dist
    from videoglamm_amd.dist import FrameSharder
    from videoglamm_amd.model import GenerationConfig, VideoGLaMMForCausalLM

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m = VideoGLaMMForCausalLM.__new__(VideoGLaMMForCausalLM)
    m.generation_config = GenerationConfig(dict(do_sample=True, temperature=0.6, top_p=0.9))
    m.comm = FrameSharder()
    torch.manual_seed(rank)                 # different RNG streams on the two ranks
    m._resolve_sampling()
    own = int(torch.empty((), dtype=torch.int64).random_())
    q.put((rank, m._sampling["seed"], own))
    dist.barrier()
    dist.destroy_process_group()


def test_seed_broadcast_world2_gloo():
    """every rank decodes with rank 0's seed, so the replicated decode draws the same ids (the kernel is deterministic given seed and logits)"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_seed_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (seed, own)) for r, seed, own in (q.get(timeout=120) for _ in procs))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    torch.manual_seed(0)
    want = int(torch.empty((), dtype=torch.int64).random_())
    assert got[0][0] == got[1][0] == want and got[1][1] != got[0][1]
