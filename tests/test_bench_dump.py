"""bench.py --dump-outputs (CPU): what the timed path returned — token ids and the {frame: {object: mask}} dict — written as float32 /
float64 .npy files under 64 MB, with the same mask sample from run to run."""
import os

import numpy as np
import torch

import bench
from videoglamm_amd.model import VideoGLaMMForCausalLM


def _segs(T, N, H, W, seed):
    m = (torch.rand(T, N, H, W, generator=torch.Generator().manual_seed(seed)) > 0.5).to(torch.uint8)
    return m, [VideoGLaMMForCausalLM._segments(m)]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_c2_sized_clip(tmp_path):
    """32 x 1 x 1024^2 masks (config C2): ids whole, areas whole, a fixed sample of the pixels; float dtypes only, < 64 MB"""
    m, segs = _segs(32, 1, 1024, 1024, 0)
    ids = torch.arange(3400)[None]
    bench.dump_outputs(str(tmp_path / "a"), ids, segs)
    bench.dump_outputs(str(tmp_path / "b"), ids, segs)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"output_ids", "mask_frames", "mask_objects", "mask_area", "mask_sample_index", "mask_sample"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64 << 20
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a["output_ids"], ids.numpy().astype(np.float64))
    assert np.array_equal(a["mask_area"], m.sum(dim=(2, 3)).numpy().astype(np.float64))
    idx = a["mask_sample_index"].astype(np.int64)
    assert idx.size == bench.DUMP_MASK_SAMPLES and np.array_equal(a["mask_sample"], m.numpy().reshape(-1)[idx].astype(np.float32))


def test_dump_outputs_small_clip_whole_and_no_masks(tmp_path):
    """a clip under the sample size is written whole; a step that returned no masks still writes every file"""
    m, segs = _segs(3, 2, 40, 56, 1)
    bench.dump_outputs(str(tmp_path / "s"), torch.arange(12)[None], segs)
    s = _load(tmp_path / "s")
    assert np.array_equal(s["mask_sample"], m.numpy().reshape(-1).astype(np.float32))
    bench.dump_outputs(str(tmp_path / "e"), torch.arange(12)[None], [{}])
    e = _load(tmp_path / "e")
    assert e["mask_area"].shape == (0, 0) and e["mask_sample"].size == 0
