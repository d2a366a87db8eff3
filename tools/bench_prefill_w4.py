"""MXFP4 prefill measurements (profiles/w4a8_prefill.txt).
usage: python tools/bench_prefill_w4.py [reps=5] [iters=20] [out=FILE] [steps=gemm,prefill,memory]
Every GPU step is a child process of this driver under its own time limit; the driver stops at the first step that fails.
  gemm     per-launch time of the four MLP GEMM shapes of C1 / C2 (M = 1697 and 3361; gate|up N = 14336, K = 4096 with SwiGLU; down N = 4096, K = 14336
           with a residual) on ops.linear (bf16), ops.linear_f8 and ops.linear_w4a8, and of the activation quantiser (ops.quantize_fp8) on its own:
           `reps` repetitions of `iters` launches, the kernels alternating inside every repetition; median and spread (max - min) of the repetitions.
           vg_gemm_f8 is compiled from vg_gemm.hip, which the MXFP4 prefill did not touch: its column is the previous build's kernel.
  prefill  the whole prefill of tools/bench_decode.py's synthetic Llama-3-8B at S = 1697 and 3361 under prefill_gemm = bf16 / fp8 / mxfp4, alternating.
  memory   torch.cuda.memory_allocated / max_memory_allocated of that model (the bf16 state dict on the device first, as a loaded checkpoint is) after
           the decoder's construction and after a prefill and 4 decode steps under prefill_gemm = decode_weights = "mxfp4", with and without
           dense_mlp = "drop" (a process each; the peak is the whole process's, the one-time quantiser included)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
kv = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
REPS, ITERS = int(kv.get("reps", "5")), int(kv.get("iters", "20"))
LIMITS = {"gemm": 300, "prefill": 600, "memory-keep": 400, "memory-drop": 400}


def say(line):
    print(line, flush=True)
    if "out" in kv:
        with open(kv["out"], "a") as f:
            f.write(line + "\n")


def med(v):
    return f"{statistics.median(v):8.1f} us (spread {max(v) - min(v):5.1f})"


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def step_gemm():
    import torch
    from videoglamm_amd import ops
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    for M in (1697, 3361):
        for name, N, K, glu in (("gate|up", 14336, 4096, True), ("down", 4096, 14336, False)):
            rows = 2 * N if glu else N
            x = torch.randn(M, K, device=dev, generator=g).to(bf)
            w = (torch.randn(rows, K, device=dev, generator=g) * 0.02).to(bf)
            r = None if glu else torch.randn(M, N, device=dev, generator=g).to(bf)
            q, qs = ops.quantize_fp8(x)
            w8, ws = ops.quantize_fp8_rows(w)
            w4 = ops.mxfp4_pack(*ops.quantize_mxfp4_rows(w))
            fns = {"bf16 ops.linear": lambda: ops.linear(x, w, glu=glu, residual=r),
                   "fp8 ops.linear_f8": lambda: ops.linear_f8(q, qs, w8, ws, glu=glu, residual=r),
                   "mxfp4 ops.linear_w4a8": lambda: ops.linear_w4a8(q, qs, w4, glu=glu, residual=r),
                   "ops.quantize_fp8 (the activations)": lambda: ops.quantize_fp8(x)}
            t = {k: [] for k in fns}
            for f in fns.values():
                f()
            torch.cuda.synchronize()
            for _ in range(REPS):
                for k, f in fns.items():
                    t[k].append(timed(f, ITERS))
            flop = 2.0 * M * rows * K
            for k in fns:
                tf = "" if "quantize" in k else f"  {flop / statistics.median(t[k]) / 1e6:7.1f} TFLOP/s"
                say(f"M={M} {name:8s} N={N} K={K}: {k:36s} {med(t[k])}{tf}")


def _llama():
    import torch
    from videoglamm_amd import synth
    dev = torch.device("cuda:0")
    cfg = synth.videoglamm_llama3_8b()
    man = {k: v for k, v in synth.vlm_manifest(cfg).items() if k.startswith(("model.layers.", "model.embed_tokens", "model.norm", "lm_head"))}
    return cfg["llm"], synth.device_state_dict(man, dev, torch.bfloat16), dev


def step_prefill():
    import torch
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    llm, sd, dev = _llama()
    P = Params(sd, dev, torch.bfloat16)
    decs = {m: LlamaDecoder(P, dict(llm, prefill_gemm=m), 4096, use_graph=False) for m in ("bf16", "fp8", "mxfp4")}
    for S in (1697, 3361):
        x = (torch.randn(S, llm["hidden"], device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.02).to(torch.bfloat16)
        t = {m: [] for m in decs}
        for rep in range(REPS + 1):
            for m, dec in decs.items():
                dec.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.forward(x)
                torch.cuda.synchronize()
                if rep:                                   # (repetition 0 builds the mode's weights)
                    t[m].append((time.perf_counter() - t0) * 1e6)
        for m in decs:
            v = [u / 1e3 for u in t[m]]
            say(f"prefill S={S} Llama-3-8B (32 layers) prefill_gemm={m:5s}: {statistics.median(v):7.2f} ms (spread {max(v) - min(v):.2f}, {REPS} repetitions)")


def step_memory(flag):
    import torch
    from videoglamm_amd.params import Params
    from videoglamm_amd.vlm import LlamaDecoder
    llm, sd, dev = _llama()
    P = Params(sd, dev, torch.bfloat16)
    del sd
    torch.cuda.synchronize()
    loaded = torch.cuda.memory_allocated()
    dec = LlamaDecoder(P, dict(llm, prefill_gemm="mxfp4", decode_weights="mxfp4", dense_mlp=flag), 4096)
    torch.cuda.synchronize()
    built, peak_built = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()      # (the peak is never reset: it is the process's)
    x = (torch.randn(1697, llm["hidden"], device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.02).to(torch.bfloat16)
    h = dec.forward(x)
    dec.next_token(h[-1:])
    for _ in range(4):
        dec.decode_step()
    torch.cuda.synchronize()
    say(f"memory Llama-3-8B prefill_gemm=decode_weights=mxfp4 dense_mlp={flag}: state dict on the device {loaded / 2**30:.2f} GiB; after the decoder's "
        f"construction allocated {built / 2**30:.2f} GiB (max_memory_allocated so far {peak_built / 2**30:.2f}); after the prefill (S = 1697) and 4 decode "
        f"steps allocated {torch.cuda.memory_allocated() / 2**30:.2f} GiB, max_memory_allocated of the process {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")


if "step" in kv:
    {"gemm": step_gemm, "prefill": step_prefill, "memory-keep": lambda: step_memory("keep"), "memory-drop": lambda: step_memory("drop")}[kv["step"]]()
else:
    want = kv.get("steps", "gemm,prefill,memory").split(",")
    for step in [s for s in LIMITS if s.split("-")[0] in want]:
        args = [sys.executable, os.path.abspath(__file__), f"step={step}", f"reps={REPS}", f"iters={ITERS}"] + ([f"out={kv['out']}"] if "out" in kv else [])
        try:
            rc = subprocess.run(args, timeout=LIMITS[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            say(f"step {step} ended with status {rc}: stopping")
            sys.exit(1)
