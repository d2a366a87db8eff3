"""One process of the clip comparison behind DESIGN 5b "On the clip": bench.py's C2 clip (32 frames of 1024^2, one [SEG], Llama-3-8B, framewise
branch) through model.inference() with or without the run-length keywords.
usage: python tools/bench_rle_clip.py MODE [TREE] [STEPS] [out.jsonl]     (out: profiles/bench_rle_clip.jsonl of THIS tree, appended)

  MODE   plain = inference()        lean = inference(return_rle=True, return_masks=False)        rle = inference(return_rle=True)
  TREE   the checkout whose package, bench.py and built library are used (default: this one).  The parent commit is measured by exporting it
         next to this tree (git archive), building it, and running `plain` with TREE pointing there: same tool, same process shape.

A process builds the model, runs 2 warm-up steps and STEPS (default 12) steps, each between two device synchronisations on the host clock, and
writes one line: the median, min and max of its steps.  The comparison alternates processes (parent plain, lean, plain, parent plain, ...);
the spread of a variant is max - min of its processes' medians."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1]
tree = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else HERE
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 12
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(HERE, "profiles", "bench_rle_clip.jsonl")
sys.path.insert(0, tree)

import torch                                                    # noqa: E402
import videoglamm_amd                                           # noqa: E402
from videoglamm_amd import synth                                # noqa: E402
from videoglamm_amd.model import VideoGLaMMForCausalLM          # noqa: E402

assert os.path.abspath(videoglamm_amd.__file__).startswith(tree + os.sep), videoglamm_amd.__file__
spec = importlib.util.spec_from_file_location("bench_of_tree", os.path.join(tree, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    cfg = synth.videoglamm_llama3_8b()
    cfg["forced_tokens"] = {8: cfg["seg_token_idx"]}            # bench.py's C2: one [SEG], at decode step 8
    sd = synth.device_state_dict(synth.manifest(cfg), dev, torch.bfloat16)
    model = synth.install_forced_tokens(VideoGLaMMForCausalLM(sd, cfg, torch_dtype=torch.bfloat16, device=dev))
    images, context, sam, ids = bench.make_inputs(cfg, argparse.Namespace(te=16, frames=32, scaling="strong"), 1, dev)
    kw = {"plain": {}, "lean": dict(return_rle=True, return_masks=False), "rle": dict(return_rle=True)}[mode]

    def step():
        return model.inference([images], [context], [sam], ids, [(1024, 1024)], [(1024, 1024)], max_new_tokens=32, use_sam2_video_branch=False, **kw)

    for _ in range(2):
        out = step()
    del sd
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    line = {"tool": "bench_rle_clip", "tree": "this" if tree == HERE else os.path.basename(tree), "mode": mode, "steps": steps,
            "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "ms": [round(v, 3) for v in ms],
            "device": torch.cuda.get_device_name(0)}
    if mode != "plain":
        codes = out[-1][0]
        line["runs_total"] = sum(len(c["counts"]) for fr in codes.values() for c in fr.values())
        line["masks"] = sum(len(fr) for fr in codes.values())
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
